"""The plan of the aggregate calls over distinct messages (bn254_amd/csrc/bn254_aggd_plan.h): route, slot and partial counts, workspace
places and the scratch layout, compiled for the host (no HIP, no device) and compared with a restatement of DESIGN.md §10 / §10a / §10b
written from the rules, over a table of shapes.  A miscount here would show on the GPU as a memory fault or an overwritten neighbour
array, never as an assertion — so the sizes are checked where nothing can fault."""
import itertools
import json
import os
import re
import subprocess

import pytest

from tests.conftest import ws_default

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bn254_amd", "csrc")
WG = ws_default("AGGD_WG_ELEMS")
TWO_MIN_M = ws_default("AGGD_TWO_PER_PAIR_MIN_M")
W1_MAX = ws_default("AGGD_KEYED_W1_MAX_SLOTS")
SUM_WG = ws_default("AGGR_SUM_WG")
# AGGR_PART_WORDS is an expression in bn254_ws.h (one Jacobian point: three coordinates of BN_LIMBS words)
PART_WORDS = 3 * int(re.search(r"#define\s+BN_LIMBS\s+(\d+)", open(os.path.join(CSRC, "bn254_constants.h")).read()).group(1))
SCAN_WG = 256          # values per workgroup of the device-side scans, one block total each

SHIM = r'''
#include "bn254_aggd_plan.h"
#include <cstdio>
#include <cstring>
#include <string>
static std::string levels(size_t e0, size_t wg) {
  std::string s = "[";
  const size_t total = seg_levels(e0, wg, [&](size_t e, size_t off, int last) {
    char b[96]; snprintf(b, sizeof b, "%s[%zu,%zu,%d]", s.size() > 1 ? "," : "", e, off, last); s += b; });
  return s + "," + std::to_string(total) + "]";          // the levels, then what the walk returned
}
#define F(x) printf("\"" #x "\":%zu,", (size_t)p.x)
// an array's address on a null base (its offset) and, on a buffer, its distance from the base — with its element size
#define R(x) printf("\"" #x "\":[%zu,%zu,%zu],", (size_t)(uintptr_t)z.x, (size_t)((uintptr_t)b.x - base), sizeof(*z.x))
#define RF(x) printf("\"" #x "\":[%zu,%zu,%zu],", (size_t)(uintptr_t)z.f.x, (size_t)((uintptr_t)b.f.x - base), sizeof(*z.f.x))
#define FRONT RF(mx); RF(incl); RF(lo); RF(hi); RF(kincl); RF(tot); RF(first_pk); RF(first_hash)
static const uintptr_t base = 0x7000000;
int main() {
  char kind;
  size_t m, n, x[5];
  while (scanf(" %c %zu %zu %zu %zu %zu %zu %zu", &kind, &m, &n, &x[0], &x[1], &x[2], &x[3], &x[4]) == 8) {
    Carve dry(nullptr), wet((void*)base);
    if (kind == 'd') {
      const AggdPlan p = aggd_plan(m, n, x[0], x[1], x[2], x[3], (int)x[4]);
      const AggdScratch z = aggd_scratch(dry, p), b = aggd_scratch(wet, p);
      printf("{\"plan\":{");
      F(m); F(n); F(width); F(n_slots); F(n_kslots); F(e0); F(n_part); F(pbase); F(gbase); F(ws_items); F(nb);
      printf("\"route\":\"%s\"},\"scratch\":{", p.route == AGGD_SLOTS ? "slots" : p.route == AGGD_TWO_PER_PAIR ? "two_per_pair" : "per_pair");
      FRONT; R(seg0); R(pseg);
      printf("\"bytes\":[%zu,%zu]},\"levels\":{\"e0\":%s}}\n", dry.used, wet.used, levels(p.e0, AGGD_WG_ELEMS).c_str());
    } else {
      const AggrPlan p = aggr_plan(m, n, x[0], x[1], (int)x[2]);
      const AggrScratch z = aggr_scratch(dry, p), b = aggr_scratch(wet, p);
      printf("{\"plan\":{");
      F(m); F(n); F(G); F(ng); F(n_b); F(n_e); F(n_tp_max); F(wx); F(wg); F(n_slots); F(n_xslots); F(n_gslots); F(n_part); F(n_spart); F(pbase);
      F(gbase); F(cbase); F(tbase); F(ws_items);
      printf("\"nb\":%zu},\"scratch\":{", p.nb);
      FRONT; R(cnt); R(tp); R(glo); R(ghi); R(gkincl); R(pair_agg); R(xseg0); R(pseg); R(nagg); R(ebkt); R(perm); R(eseg); R(bkey); R(gseg0);
      R(spseg); R(part); R(gst); R(queued);
      printf("\"bytes\":[%zu,%zu]},\"levels\":{\"x\":%s,\"g\":%s,\"s\":%s}}\n", dry.used, wet.used, levels(p.n_xslots, AGGD_WG_ELEMS).c_str(),
             levels(p.n_gslots, AGGD_WG_ELEMS).c_str(), levels(p.n_e, AGGR_SUM_WG).c_str());
    }
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("aggd_plan")
    src, exe = out / "plan.cpp", out / "plan"
    src.write_text(SHIM)
    defs = {"AGGD_WG_ELEMS": WG, "AGGD_TWO_PER_PAIR_MIN_M": TWO_MIN_M, "AGGD_KEYED_W1_MAX_SLOTS": W1_MAX, "AGGR_SUM_WG": SUM_WG, "AGGR_PART_WORDS": PART_WORDS}
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC] + ["-D%s=%d" % kv for kv in defs.items()]
                          + ["-o", str(exe), str(src)])

    def run(rows):
        text = "".join("%s %s\n" % (r[0], " ".join(str(int(v)) for v in list(r[1:]) + [0] * (8 - len(r)))) for r in rows)
        got = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600, check=True).stdout.splitlines()
        assert len(got) == len(rows)
        return [json.loads(line) for line in got]
    return run


# ---- the rules, restated -------------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def up256(x):
    return ceil_div(x, 256) * 256


def partials(e, wg):
    """a level of e elements runs ceil(e / wg) workgroups; more than one: each leaves two partials, and those are the next level's elements"""
    groups = ceil_div(e, wg)
    return 0 if groups <= 1 else 2 * groups + partials(2 * groups, wg)


def width_rule(knob, table_pairs_bound):
    """§10a: one table pair per lane pair while they fit one pass (AGGD_KEYED_W1_MAX_SLOTS), else two; the knob's 1 / 2 force it"""
    return knob if knob in (1, 2) else 1 if table_pairs_bound <= W1_MAX else 2


def keyed_slots(width, pairs, aggs):
    """the bound on sum of ceil((k_i + 1) / width) over `aggs` disjoint ranges holding `pairs` pairs in all"""
    return pairs + aggs if width == 1 else pairs // 2 + aggs


def exact_plan(m, n, keyed, have_keys, pair_lanes, lane_machine, knob):
    if keyed and m > 0 and have_keys and pair_lanes and knob != 3:
        route = "slots"
    elif not pair_lanes or lane_machine or m < TWO_MIN_M:
        route = "per_pair"
    else:
        route = "two_per_pair"
    width = width_rule(knob, m + n) if route == "slots" else 0
    n_slots = ceil_div(m + n, 2)
    n_kslots = keyed_slots(width, m, n) if route == "slots" else 0
    e0 = {"slots": n_kslots, "per_pair": m, "two_per_pair": n_slots}[route]
    n_part = partials(e0, WG)
    pbase = up256(m)
    gbase = up256(max(pbase + n_part, n))
    plan = dict(m=m, n=n, route=route, width=width, n_slots=n_slots, n_kslots=n_kslots, e0=e0, n_part=n_part, pbase=pbase, gbase=gbase,
                ws_items=gbase + n, nb=ceil_div(n, SCAN_WG))
    front = dict(mx=(8, n), incl=(8, n), lo=(8, n), hi=(8, n), kincl=(8, n if route == "slots" else 0), tot=(8, plan["nb"]), first_pk=(4, n), first_hash=(4, n))
    return plan, dict(front, seg0=(4, e0), pseg=(4, n_part))


def rand_plan(m, n, K, group_pairs, knob):
    G = max(group_pairs, K)
    ng = m // G + 1
    n_tp_max = min(m, ng * K)
    wx, wg = width_rule(knob, m + n), width_rule(0, n_tp_max + ng)
    n_xslots, n_gslots = keyed_slots(wx, m, n), keyed_slots(wg, n_tp_max, ng)
    n_part, n_spart = max(partials(n_xslots, WG), partials(n_gslots, WG)), partials(m + n, SUM_WG)
    pbase = up256(m + 1)
    gbase = up256(max(pbase + n_part, n))
    cbase = up256(gbase + n)
    tbase = up256(cbase + ng)
    plan = dict(m=m, n=n, G=G, ng=ng, n_b=ng * (K + 1), n_e=m + n, n_tp_max=n_tp_max, wx=wx, wg=wg, n_slots=ceil_div(m + n, 2), n_xslots=n_xslots,
                n_gslots=n_gslots, n_part=n_part, n_spart=n_spart, pbase=pbase, gbase=gbase, cbase=cbase, tbase=tbase, ws_items=tbase + n_tp_max,
                nb=ceil_div(max(n, ng * (K + 1), ng), SCAN_WG))
    n_e, n_b = m + n, plan["n_b"]
    scratch = dict(mx=(8, n), incl=(8, n), lo=(8, n), hi=(8, n), kincl=(8, n), tot=(8, plan["nb"]), first_pk=(4, n), first_hash=(4, n),
                   cnt=(8, n_b), tp=(8, n_b), glo=(8, ng), ghi=(8, ng), gkincl=(8, ng), pair_agg=(4, m), xseg0=(4, n_xslots), pseg=(4, n_part),
                   nagg=(4, ng), ebkt=(4, n_e), perm=(4, n_e), eseg=(4, n_e), bkey=(4, tbase + n_tp_max), gseg0=(4, n_gslots), spseg=(4, n_spart),
                   part=(4, PART_WORDS * n_spart), gst=(1, ng), queued=(1, n))
    return plan, scratch


# ---- the shapes ----------------------------------------------------------------------------------------------------------------------------
RAGGED = [[1], [0, 1, 2, 3], [5, 0, 0, 130, 1, 257, 2], [64] * 3 + [1] * 9, [2] * 100 + [3] * 33]       # pairs per aggregate
SHAPES = sorted(set(
    [(0, 1), (0, 5), (1, 1)] + [(sum(k), len(k)) for k in RAGGED]
    + [(W1_MAX - n + d, n) for n in (1, 4, 4096) for d in (-1, 0, 1)]                                     # m + n at the width rule
    + [(TWO_MIN_M + d, n) for n in (1, 16) for d in (-1, 0, 1)]                                           # m at the two-per-pair threshold
    + [(e + d, 1) for e in (WG, WG * 64) for d in (-2, -1, 0, 1)]                                      # e0 = m and e0 = m + n around 128, 129, 128 * 64
    + [(2 * (e + d) - 1, 1) for e in (WG, WG * 64) for d in (-1, 0, 1)]                                   # e0 = (m + n + 1) / 2 and m / 2 + n around them
    + [(1 << 20, 1), ((1 << 20) - 1, 1), ((1 << 21) - 1, 1), (4096 * 16, 4096), (65536, 65536)]))         # e0 = 2^20 on every route


def check_scratch(got, want):
    """(b): regions pairwise disjoint, aligned to their element, inside the reported byte count; the same on a null base and on a buffer"""
    dry_bytes, wet_bytes = got.pop("bytes")
    assert dry_bytes == wet_bytes
    assert set(got) == set(want)
    spans = []
    for name, (off, off_on_buffer, elem) in got.items():
        size, count = want[name]
        assert elem == size and off % size == 0 and off == off_on_buffer, name
        spans.append((off, off + size * count, name))
    spans.sort()
    for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
        assert end <= start, (a, b)
    assert spans[-1][1] <= dry_bytes
    assert dry_bytes - sum(size * count for size, count in want.values()) < 8 * len(want)      # nothing but alignment padding


def check_levels(walk, e0, wg, n_part):
    """(d): the walk starts at e0, every level's partials follow the level before, the last level is one workgroup, n_part entries in all"""
    *levels, total = walk
    e, off = e0, 0
    for i, (got_e, got_off, last) in enumerate(levels):
        assert (got_e, got_off) == (e, off)
        groups = ceil_div(e, wg)
        assert bool(last) == (i == len(levels) - 1) == (groups <= 1)
        e, off = 2 * groups, off + (0 if last else 2 * groups)
    assert total == off == partials(e0, wg) and total <= n_part


def test_exact_plans(shim):
    rows = [("d", m, n, keyed, keys, lanes, lm, knob) for (m, n), keyed, keys, lanes, knob in itertools.product(SHAPES, (0, 1), (0, 1), (0, 1), range(4))
            for lm in ((0, 1) if lanes else (0,))]                              # the lane machine is a layout of the lane pairs
    routes = set()
    for row, got in zip(rows, shim(rows)):
        plan, scratch = exact_plan(*row[1:])
        assert got["plan"] == plan, row                                         # (a)
        check_scratch(got["scratch"], scratch)                                  # (b)
        m, n = row[1:3]
        assert m <= plan["pbase"] and plan["pbase"] + plan["n_part"] <= plan["gbase"] and plan["gbase"] + n <= plan["ws_items"]     # (c)
        check_levels(got["levels"]["e0"], plan["e0"], WG, plan["n_part"])
        assert partials(plan["e0"], WG) == plan["n_part"]
        routes.add((plan["route"], plan["width"]))
    assert routes == {("slots", 1), ("slots", 2), ("two_per_pair", 0), ("per_pair", 0)}
    e0s = {exact_plan(m, n, k, 1, 1, 0, 0)[0]["e0"] for m, n in SHAPES for k in (0, 1)} | {exact_plan(m, n, 0, 0, 0, 0, 0)[0]["e0"] for m, n in SHAPES}
    assert {WG - 1, WG, WG + 1, WG * 64 - 1, WG * 64, WG * 64 + 1, 1 << 20} <= e0s


def test_randomised_plans(shim):
    rows = [("r", m, n, K, G, knob) for (m, n), K, G, knob in itertools.product(SHAPES, (1, 256, 1024), (68, 200, 1024, 4096), range(4))]
    for row, got in zip(rows, shim(rows)):
        plan, scratch = rand_plan(*row[1:])
        assert got["plan"] == plan, row
        check_scratch(got["scratch"], scratch)
        m, n = row[1:3]
        assert m + 1 <= plan["pbase"] and plan["pbase"] + plan["n_part"] <= plan["gbase"] and plan["gbase"] + n <= plan["cbase"]
        assert plan["cbase"] + plan["ng"] <= plan["tbase"] and plan["tbase"] + plan["n_tp_max"] == plan["ws_items"]
        assert scratch["bkey"] == (4, plan["tbase"] + plan["n_tp_max"])        # indexed by workspace position
        check_levels(got["levels"]["x"], plan["n_xslots"], WG, plan["n_part"])
        check_levels(got["levels"]["g"], plan["n_gslots"], WG, plan["n_part"])
        check_levels(got["levels"]["s"], plan["n_e"], SUM_WG, plan["n_spart"])
        assert max(partials(plan["n_xslots"], WG), partials(plan["n_gslots"], WG)) == plan["n_part"] and partials(plan["n_e"], SUM_WG) == plan["n_spart"]


@pytest.mark.parametrize("sizes", RAGGED + [[0] * 7, [1] * 300, [3, 1] * 50])
def test_slot_bounds_hold_for_disjoint_ranges(sizes):
    """the host-known bounds the plans size by: the slots of two pairs and the slot kernel's slots of real ranges never exceed them"""
    m, n = sum(sizes), len(sizes)
    assert sum(ceil_div(k, 2) for k in sizes) <= exact_plan(m, n, 0, 0, 1, 0, 0)[0]["n_slots"]
    for width in (1, 2):
        assert sum(ceil_div(k + 1, width) for k in sizes) <= keyed_slots(width, m, n)
