"""The subset-sum tables of the aggregate verify's pools (bn254_amd/csrc/bn254_pooltab.h: the per-lane bodies of k_pool_subsets_g2 / _g1,
k_pool_pairs_g1, k_pool_quads_g1, k_pool_widen_g1 / _g2), without a GPU: compiled for the host (tests/hostsim/hostsim_pooltab.cpp) in the
one-lane layout the builders run in, lane after lane, plain and under -DBN_TRACK_BOUNDS.
- plain: EVERY entry and identity flag of T8 keys, T2, T4, T8 signatures and T16 keys, for pools of 5, 8, 16, 17 and 43 signers over two
  messages (tests/pooltab_cases.py), equals the oracle's sum of the selected signers; T4 built both ways (pairs + quads, and every entry
  from the pool) gives the same points; a lane past the end of a launch stores nothing.
- bounds: the whole chain on the planted 43-signer pool, and one lane of the widening per flow (a regular chord, B = A, B = -A, an
  identity A, an identity B; Fq and Fq2; batches of 4 and 8), under the interval tracker with the stored-word contract checked at every
  store and assumed at every load — an induction over the chained stages, not one run; and the consumer's side in the pair layout
  (jac_from_affine, jac_accumulate_from on records loaded under the contract, as k_aggregate_pair runs them).
- the contract check is not vacuous: an unreduced store aborts with a BOUND VIOLATION.
- the option and the hook of the library are declared, numbered, exported and bound."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from bn254_amd import _native
from tests import pooltab_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_pooltab.cpp")


def test_option_and_hook_declared():
    from bn254_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert re.search(r"#define BN254_OPT_AGG_T4_ROUTE 42\b", hdr) and engine.OPT_AGG_T4_ROUTE == 42
    m = re.search(r"\bint\s+bn254_debug_agg_tables\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 6 and "bn254_debug_agg_tables" in _native.EXPORTED_SYMBOLS
    assert hdr.index("#ifndef BN254_NO_DEV_HOOKS") < m.start() and hdr.index("#ifndef BN254_NO_DEV_HOOKS") < hdr.index("BN254_OPT_AGG_T4_ROUTE")
    _native.build()
    assert len(_native.load().bn254_debug_agg_tables.argtypes) == 6
    # the kernels are wrappers: the arithmetic of the builders lives in the header the host compilation reads
    group = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_group.hip")).read()
    for lane in ("pt_subsets_g2_lane", "pt_subsets_g1_lane", "pt_pairs_g1_lane", "pt_quads_g1_lane", "pt_widen_g1_lane", "pt_widen_g2_lane"):
        assert lane + "(" in group, lane
    assert "aff_add_given_inv" not in group and "pool_widen_lane" not in group.replace("bn254_pooltab.h: pool_widen_lane", "")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("hp")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"], "consumer": ["-O1", "-DBN_TRACK_BOUNDS", "-DPT_PAIR_CONSUMER"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhp_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


class Harness:
    def __init__(self, path):
        self.lib = L = ctypes.CDLL(path)
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.hp_build.argtypes = [sz, sz, vp, vp, vp, vp, i32]
        L.hp_build.restype = None
        L.hp_entries.argtypes = [i32]
        L.hp_entries.restype = sz
        L.hp_read.argtypes = [i32, sz, sz, vp, vp]
        L.hp_flow.argtypes = [i32, i32, vp, vp, vp, vp]

    def build(self, P, t4_route=0):
        self.lib.hp_build(pc.M, P.S, P.pk_pool, bytes(P.pk_st), P.sig_pool, bytes(st for row in P.sig_st for st in row), t4_route)
        assert self.lib.hp_canaries_ok() == 1                 # the lane past the end of every launch stored nothing

    def read(self, which, first, count):
        size = 128 if which in (0, 3, 5) else 64
        pts, fl = ctypes.create_string_buffer(count * size), ctypes.create_string_buffer(count)
        assert self.lib.hp_read(which, first, count, pts, fl) == 0
        return pts.raw, fl.raw

    def flow(self, g2, batch, a, bs):
        size = 128 if g2 else 64
        out, fl = ctypes.create_string_buffer(batch * size), ctypes.create_string_buffer(batch)
        assert self.lib.hp_flow(g2, batch, a, b"".join(bs), out, fl) == 0
        return [out.raw[size * i:size * (i + 1)] for i in range(batch)], fl.raw


def check_tables(h, S, tables=("T8k", "T2", "T4", "T8s", "T16")):
    """every entry and every flag of the named tables against the oracle's sums"""
    P = pc.pool(S)
    for table in tables:
        which, W, g2 = pc.TABLES[table]
        assert h.lib.hp_entries(which) == (1 if g2 else pc.M) * P.windows(table) << W, table
        for m in range(1 if g2 else pc.M):
            for w in range(P.windows(table)):
                want_pts, want_fl = pc.expected(S, table, w, m)
                got_pts, got_fl = h.read(which, pc.entry_base(S, table, w, m), 1 << W)
                assert got_fl == want_fl, (S, table, m, w)
                if got_pts != want_pts:
                    size = 128 if g2 else 64
                    bad = [i for i in range(1 << W) if got_pts[size * i:size * (i + 1)] != want_pts[size * i:size * (i + 1)]]
                    raise AssertionError((S, table, m, w, len(bad), bad[:8]))


def test_planted_pool_reaches_every_exceptional_category():
    """a pool that misses a category must fail, not pass: from the secret keys alone, every widening stage of the 43-signer pool meets
    equal operands and opposite operands at least once, and the pair builder a doubling and a cancellation"""
    counts = pc.exceptional_counts(43)
    assert set(counts) == {"T2->T4", "T4->T8", "T8->T16"}
    for stage, (eq, op) in counts.items():
        assert eq >= 1 and op >= 1, (stage, eq, op)
    dbl, can = pc.pair_counts(43)
    assert dbl >= 1 and can >= 1
    P = pc.pool(43)
    k = P.sks
    # the planted relations hold as planted (a later edit of PLANTED that breaks an earlier line would show here)
    assert k[10] == (k[8] + k[9]) % pc.R and k[11] == pc.neg_scalar(k[10]) and k[12] == (k[0] + k[2]) % pc.R and k[13] == pc.neg_scalar((k[4] + k[5]) % pc.R)
    assert (k[12] + k[13]) % pc.R == (k[14] + k[15]) % pc.R and k[22] == (k[16] + k[18]) % pc.R and k[23] == pc.neg_scalar((k[17] + k[19]) % pc.R)
    assert (k[28] + k[29]) % pc.R == (k[24] + k[26]) % pc.R and (k[30] + k[31]) % pc.R == (k[16] + k[17]) % pc.R
    assert k[32] == k[0] and k[33] == pc.neg_scalar(k[2]) and k[1] == k[0] and k[3] == pc.neg_scalar(k[2])
    # the identity key, the key and the signature that do not decode: the identity in every table
    for table, signer, msgs in (("T8k", pc.IDENTITY_SIGNER, (0,)), ("T8k", pc.BAD_KEY_SIGNER, (0,)), ("T2", pc.IDENTITY_SIGNER, (0, 1)), ("T2", pc.BAD_SIG_SIGNER, (1,))):
        W = pc.TABLES[table][1]
        for m in msgs:
            assert pc.scalars(43, table, signer // W, m)[1 << (signer % W)] == 0
    assert pc.scalars(43, "T2", pc.BAD_SIG_SIGNER // 2, 0)[1 << (pc.BAD_SIG_SIGNER % 2)] != 0      # ... of that one message only


@pytest.mark.parametrize("S", pc.SIZES)
def test_every_entry_of_every_table_against_the_oracle(libs, S):
    h = Harness(libs["plain"])
    P = pc.pool(S)
    h.build(P, 0)
    check_tables(h, S)
    # the decoded pools the hook also hands out: flags = decode status | identity
    fk, fs = P.decoded_flags()
    assert h.read(0, 0, S)[1] == fk and h.read(1, 0, pc.M * S)[1] == fs
    quads = h.read(4, 0, h.lib.hp_entries(4))
    # T4 straight from the pool (k_pool_subsets_g1's body): the same points and flags, and the same T8 signatures on top of it
    h.build(P, 1)
    assert h.lib.hp_entries(7) == 0
    assert h.read(4, 0, h.lib.hp_entries(4)) == quads
    check_tables(h, S, ("T4", "T8s"))


FLOW_KINDS = ["regular", "B=A", "B=-A", "identity_A", "identity_B"]


def flow_operands(c, g2, batch, kind, rnd):
    """-> (A, [B_i], [A + B_i]) with the flow's special operand at a batch position of its own and ordinary points elsewhere"""
    gen = c.g2_generator() if g2 else c.g1_generator()
    mul, add, zero = (c.g2_mul, c.g2_add, pc.G2_ID) if g2 else (c.g1_mul, c.g1_add, pc.G1_ID)
    ka = rnd.randrange(1, pc.R)
    a = zero if kind == "identity_A" else mul(gen, ka.to_bytes(32, "big"))
    bs = [mul(gen, rnd.randrange(1, pc.R).to_bytes(32, "big")) for _ in range(batch)]
    for pos in {0, batch - 1, rnd.randrange(batch)}:                       # i == 0 (dinv = inv) and the last position are paths of their own
        if kind == "B=A":
            bs[pos] = a
        elif kind == "B=-A":
            bs[pos] = mul(gen, pc.neg_scalar(ka).to_bytes(32, "big"))
        elif kind == "identity_B":
            bs[pos] = zero
    if kind != "regular":
        bs[1] = mul(gen, rnd.randrange(1, pc.R).to_bytes(32, "big"))         # one ordinary entry shares the batch's inversion
    want = [b if a == zero else a if b == zero else add(a, b) for b in bs]
    return a, bs, want


def run_flows(h, g2, batch):
    import random
    from oracle import c_oracle as c
    rnd = random.Random(1000 * g2 + batch)
    for kind in FLOW_KINDS:
        a, bs, want = flow_operands(c, g2, batch, kind, rnd)
        got, fl = h.flow(g2, batch, a, bs)
        assert got == want, (kind, [i for i in range(batch) if got[i] != want[i]])
        assert fl == bytes(0x80 if w == (pc.G2_ID if g2 else pc.G1_ID) else 0 for w in want), kind
        if kind == "B=-A":
            assert fl[0] == 0x80 and fl[batch - 1] == 0x80 and fl[1] == 0


@pytest.mark.parametrize("build", ["plain", "bounds"])
@pytest.mark.parametrize("g2", [0, 1])
@pytest.mark.parametrize("batch", [4, 8])
def test_widening_flows(libs, build, g2, batch):
    """one lane of pool_widen_lane per flow; under `bounds` every operand is loaded and every result stored under the contract (in a process
    of its own: a violation aborts it)"""
    if build == "plain":
        run_flows(Harness(libs[build]), g2, batch)
    else:
        p = run_driver(libs[build], "flows", str(g2), str(batch))
        assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout[-500:], p.stderr[-3000:])


DRIVER = r'''
import sys
sys.path.insert(0, sys.argv[1])
from tests import pooltab_cases as pc
from tests.test_aggregate_pool_tables import Harness, check_tables, run_consumer, run_flows
which = sys.argv[3]
h = Harness(sys.argv[2]) if which != "consume" else None
if which == "consume":
    run_consumer(sys.argv[2], int(sys.argv[4]))
elif which == "chain":
    for route in (0, 1):
        h.build(pc.pool(43), route)
        check_tables(h, 43, ("T2", "T4", "T8s", "T8k") if route == 0 else ("T4",))
elif which == "flows":
    run_flows(h, int(sys.argv[4]), int(sys.argv[5]))
elif which == "unsafe":
    h.lib.hp_unsafe_store()
print("ok")
'''


def run_driver(lib, which, *args):
    return subprocess.run([sys.executable, "-c", DRIVER, ROOT, lib, which] + list(args), capture_output=True, text=True, timeout=900)


def test_bounds_hold_along_the_chain(libs):
    """decoded pools -> T8 keys -> T16, and -> T2 -> T4 -> T8 signatures (and T4 from the pool), on the pool with every planted category,
    under the tracker: every load assumes the contract, every store proves it for the next stage.  (A violation aborts the process.)"""
    p = run_driver(libs["bounds"], "chain")
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout[-500:], p.stderr[-3000:])


def test_contract_check_is_not_vacuous(libs):
    p = run_driver(libs["bounds"], "unsafe")
    assert p.returncode != 0 and "BOUND VIOLATION" in p.stderr and "stored-word contract" in p.stderr
    assert run_driver(libs["plain"], "unsafe").returncode == 0               # the plain build has no tracker: the same call returns


def run_consumer(path, g2):
    import random
    from oracle import c_oracle as c
    L = ctypes.CDLL(path)
    L.hp_consume.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.hp_consume.restype = None
    rnd = random.Random(77 + g2)
    gen = c.g2_generator() if g2 else c.g1_generator()
    mul, add, zero, size = (c.g2_mul, c.g2_add, pc.G2_ID, 128) if g2 else (c.g1_mul, c.g1_add, pc.G1_ID, 64)
    k = [rnd.randrange(1, pc.R) for _ in range(4)]
    pt = lambda s: mul(gen, (s % pc.R).to_bytes(32, "big")) if s % pc.R else zero      # noqa: E731
    for scal in ([k[0], k[1], k[2]], [k[0], 0, k[1]], [0, k[0], k[1]], [k[0], k[0], k[1]], [k[0], k[1], k[0] + k[1], k[2]],
                 [k[0], -k[0], k[1], k[2]], [k[0], k[1], -(k[0] + k[1])], [k[3]]):
        recs = [pt(s) for s in scal]
        want = zero
        for r in recs:
            want = r if want == zero else want if r == zero else add(want, r)
        out = ctypes.create_string_buffer(size)
        L.hp_consume(g2, b"".join(recs), len(recs), out)
        assert out.raw == want == pt(sum(scal)), scal


@pytest.mark.parametrize("g2", [0, 1])
def test_consumer_additions_hold_under_the_contract(libs, g2):
    """k_aggregate_pair's additions on table records, pair layout, under the tracker (a process of its own): the seed (jac_from_affine),
    ordinary additions, an identity record, a record equal to the running sum (the complete formula's doubling) and one opposite to it (the
    sum becomes the identity, and the next addition starts from it) — every record loaded under the stored-word contract"""
    p = run_driver(libs["consumer"], "consume", str(g2))
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout[-500:], p.stderr[-3000:])
