// The plan of an aggregate verify over distinct messages (bn254_aggdist.hip): the route, the element counts of
// the reduction levels, the places in the workspace and the scratch layout — arithmetic on sizes in plain C++ (no HIP, no field types).  The
// library includes it after bn254_ws.h, whose AGGD_WG_ELEMS, AGGD_TWO_PER_PAIR_MIN_M, AGGD_KEYED_W1_MAX_SLOTS, AGGR_SUM_WG and
// AGGR_PART_WORDS it uses; tests/test_aggd_plan.py compiles it for the host with those five given by -D.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#define AGGD_SCAN_WG 256                            // the device-side scans over the aggregates: values per workgroup, one block total each
static inline size_t aggd_round256(size_t x) { return (x + 255) & ~(size_t)255; }
// The levels of a segmented reduction: a level of e elements runs ceil(e / wg) workgroups and, unless that is one, leaves two partials
// each for the next level.  fn(e, off, last) per level — its partials go to entry `off` of the partial array; returns the entries needed.
template <class Fn>
static inline size_t seg_levels(size_t e, size_t wg, Fn fn) {
  for (size_t off = 0;;) {
    const size_t g = (e + wg - 1) / wg;
    const int last = g <= 1;
    fn(e, off, last);
    if (last) return off;
    e = 2 * g;
    off += 2 * g;
  }
}
static inline size_t seg_partials(size_t e, size_t wg) { return seg_levels(e, wg, [](size_t, size_t, int) {}); }
// the slot kernel on the registered tables: one table pair per lane pair while `bound` of them fit one pass of two waves per SIMD, else
// two (knob: BN254_OPT_AGGD_KEYED_ROUTE, 1 / 2 force the width); an aggregate of k pairs has k + 1 table pairs, sigma's included,
// so over disjoint ranges the slots ceil((k_i + 1) / width) number at most pairs + aggs resp. pairs / 2 + aggs
static inline int aggd_keyed_width(int knob, size_t bound) { return knob == 1 || knob == 2 ? knob : bound <= AGGD_KEYED_W1_MAX_SLOTS ? 1 : 2; }
static inline size_t aggd_keyed_slots(int width, size_t pairs, size_t aggs) { return width == 1 ? pairs + aggs : pairs / 2 + aggs; }

// a buffer handed out array by array, each aligned to its element: on a null base the addresses are offsets and `used` ends as the byte
// count; on the buffer they are the pointers.  One layout function run twice, so the size and the pointers cannot disagree.
struct Carve {
  uintptr_t base;
  size_t used = 0;
  explicit Carve(void* buf) : base((uintptr_t)buf) {}
  template <class T> T* take(size_t count) {
    used = (used + alignof(T) - 1) & ~(alignof(T) - 1);
    T* r = (T*)(base + used);
    used += count * sizeof(T);
    return r;
  }
};
// what steps 1-3 write per aggregate: the prefix maximum of the offsets, the inclusive scans of the slot counts (two pairs a slot; kincl:
// the slot kernel's), the accepted pair range, the scans' block totals, the first failing key and message
struct AggdFrontBufs { uint64_t *mx, *incl, *lo, *hi, *kincl, *tot; uint32_t *first_pk, *first_hash; };
static inline AggdFrontBufs aggd_front_bufs(Carve& c, size_t n, size_t n_kincl, size_t nb) {
  AggdFrontBufs f;
  f.mx = c.take<uint64_t>(n), f.incl = c.take<uint64_t>(n), f.lo = c.take<uint64_t>(n), f.hi = c.take<uint64_t>(n);
  f.kincl = c.take<uint64_t>(n_kincl);
  f.tot = c.take<uint64_t>(nb);
  f.first_pk = c.take<uint32_t>(n), f.first_hash = c.take<uint32_t>(n);
  return f;
}

// ---- the exact calls (§10, §10a) -----------------------------------------------------------------------------------------------------------
// level 0: the slot kernel on the registered tables; the segmented Miller kernel (two pairs of an aggregate per lane pair, the first product
// fused); or one Miller loop per pair (lane machine, lane pairs, or one lane) followed by the level kernel over the pairs
enum AggdRoute { AGGD_SLOTS, AGGD_TWO_PER_PAIR, AGGD_PER_PAIR };
struct AggdPlan {
  size_t m, n;
  AggdRoute route;
  int width;                           // table pairs per slot (AGGD_SLOTS), else 0
  size_t n_slots, n_kslots;            // slots of two pairs, sum of ceil(k_i / 2) <= (m + n + 1) / 2; the slot kernel's
  size_t e0, n_part;                   // elements of level 0; partial entries of all levels
  size_t pbase, gbase, ws_items, nb;   // workspace: pairs from 0, partials from pbase, aggregates from gbase; block totals of a scan over n
};
// keyed with keys registered, pair lanes on and route_knob != 3: the slot kernel at every size (sigma's pair in a slot like any other: no
// tail) — it beats the expanded keys on the lane machine too, whose sigma tail is a whole Miller loop.  Else the unkeyed
// call's route (a keyed call expands its keys into the Q planes): per pair on the lane machine (smallest m: latency), with pair lanes off
// and below AGGD_TWO_PER_PAIR_MIN_M (one pair per lane pair fills the chip), else two per lane pair.  No pairs: per pair, nothing to run.
static inline AggdPlan aggd_plan(size_t m, size_t n, bool keyed, bool have_keys, bool pair_lanes, bool lane_machine, int route_knob) {
  AggdPlan p = {m, n};
  p.route = keyed && m && pair_lanes && have_keys && route_knob != 3 ? AGGD_SLOTS
            : lane_machine || !pair_lanes || m < AGGD_TWO_PER_PAIR_MIN_M ? AGGD_PER_PAIR : AGGD_TWO_PER_PAIR;
  p.width = p.route == AGGD_SLOTS ? aggd_keyed_width(route_knob, m + n) : 0;
  p.n_slots = (m + n + 1) / 2;
  p.n_kslots = p.route == AGGD_SLOTS ? aggd_keyed_slots(p.width, m, n) : 0;
  p.e0 = p.route == AGGD_SLOTS ? p.n_kslots : p.route == AGGD_PER_PAIR ? m : p.n_slots;
  p.n_part = seg_partials(p.e0, AGGD_WG_ELEMS);
  p.pbase = aggd_round256(m);
  p.gbase = aggd_round256(std::max(p.pbase + p.n_part, n));
  p.ws_items = p.gbase + n;
  p.nb = (n + AGGD_SCAN_WG - 1) / AGGD_SCAN_WG;
  return p;
}
struct AggdScratch { AggdFrontBufs f; uint32_t *seg0, *pseg; };   // level 0's element -> aggregate (per-pair route: pair -> aggregate); the partials' ids
static inline AggdScratch aggd_scratch(Carve& c, const AggdPlan& p) {
  AggdScratch b;
  b.f = aggd_front_bufs(c, p.n, p.route == AGGD_SLOTS ? p.n : 0, p.nb);
  b.seg0 = c.take<uint32_t>(p.e0);
  b.pseg = c.take<uint32_t>(p.n_part);
  return b;
}

// ---- randomised, against registered keys (§10b) ----------------------------------------------------------------------------------------------
struct AggrPlan {
  size_t m, n;
  size_t G, ng, n_b, n_e;              // messages per group, groups, (group, key) buckets with the signatures' (K + 1 a group), entries
  int wx, wg;                          // slot widths: the re-check (the exact call's rule), the group checks (the same rule on their bound)
  size_t n_slots, n_xslots, n_gslots;
  size_t n_part, n_spart;              // partial entries: the larger of the two checks' Fq12 products; the G1 sums
  size_t pbase, gbase, cbase, tbase, ws_items;   // workspace: ... aggregates from gbase, groups (S_g, their products) from cbase, table pairs from tbase
  size_t n_tp_max, nb;                 // table pairs: one per non-empty (group, key) bucket; block totals of the longest scan (n, n_b or ng values)
};
static inline AggrPlan aggr_plan(size_t m, size_t n, size_t K, size_t group_pairs, int route_knob) {
  AggrPlan p = {m, n};
  p.G = std::max(group_pairs, K);
  p.ng = m / p.G + 1;
  p.n_b = p.ng * (K + 1);
  p.n_e = m + n;
  p.n_tp_max = m < p.ng * K ? m : p.ng * K;
  p.wx = aggd_keyed_width(route_knob, m + n);
  p.wg = aggd_keyed_width(0, p.n_tp_max + p.ng);
  p.n_slots = (m + n + 1) / 2;
  p.n_xslots = aggd_keyed_slots(p.wx, m, n);
  p.n_gslots = aggd_keyed_slots(p.wg, p.n_tp_max, p.ng);
  p.n_part = std::max(seg_partials(p.n_xslots, AGGD_WG_ELEMS), seg_partials(p.n_gslots, AGGD_WG_ELEMS));
  p.n_spart = seg_partials(p.n_e, AGGR_SUM_WG);
  p.pbase = aggd_round256(m + 1);
  p.gbase = aggd_round256(std::max(p.pbase + p.n_part, n));
  p.cbase = aggd_round256(p.gbase + n);
  p.tbase = aggd_round256(p.cbase + p.ng);
  p.ws_items = p.tbase + p.n_tp_max;
  p.nb = (std::max(std::max(n, p.n_b), p.ng) + AGGD_SCAN_WG - 1) / AGGD_SCAN_WG;
  return p;
}
struct AggrScratch {
  AggdFrontBufs f;
  uint64_t *cnt, *tp, *glo, *ghi, *gkincl;     // per bucket: entries, then table-pair ranks; per group: its table pairs [glo, ghi), its slot scan
  uint32_t *pair_agg, *xseg0, *pseg, *nagg, *ebkt, *perm, *eseg, *bkey, *gseg0, *spseg;
  int32_t* part;                               // the G1 sums' partials, AGGR_PART_WORDS each
  uint8_t *gst, *queued;
};
static inline AggrScratch aggr_scratch(Carve& c, const AggrPlan& p) {
  AggrScratch b;
  b.f = aggd_front_bufs(c, p.n, p.n, p.nb);
  b.cnt = c.take<uint64_t>(p.n_b), b.tp = c.take<uint64_t>(p.n_b);
  b.glo = c.take<uint64_t>(p.ng), b.ghi = c.take<uint64_t>(p.ng), b.gkincl = c.take<uint64_t>(p.ng);
  b.pair_agg = c.take<uint32_t>(p.m);
  b.xseg0 = c.take<uint32_t>(p.n_xslots);
  b.pseg = c.take<uint32_t>(p.n_part);
  b.nagg = c.take<uint32_t>(p.ng);
  b.ebkt = c.take<uint32_t>(p.n_e), b.perm = c.take<uint32_t>(p.n_e), b.eseg = c.take<uint32_t>(p.n_e);
  b.bkey = c.take<uint32_t>(p.tbase + p.n_tp_max);   // indexed by workspace position: a table pair's key beside its point
  b.gseg0 = c.take<uint32_t>(p.n_gslots);
  b.spseg = c.take<uint32_t>(p.n_spart);
  b.part = c.take<int32_t>(AGGR_PART_WORDS * p.n_spart);
  b.gst = c.take<uint8_t>(p.ng), b.queued = c.take<uint8_t>(p.n);
  return b;
}
