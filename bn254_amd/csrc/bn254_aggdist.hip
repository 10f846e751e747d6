// Translation unit of libbn254hip.so: aggregate verification over DISTINCT messages (include/bn254_hip.h:
// bn254_batch_aggregate_verify_distinct[_device]) — the host side and the one-lane bookkeeping kernels.  Aggregate i owns the pairs
// j in [agg_off[i], agg_off[i+1]) and passes iff  e(sigma_i, -G2::one()) * prod_j e(H(m_j), pk_j) == 1  (the IRTF draft's AggregateVerify;
// the sums are the reference's `Add for Signature`, src/types.rs:264-270; the check is ECDSA::verify's, src/ecdsa.rs:49-64).
//
// Workspace: pair j at index j (key: Q planes, H(m_j): P1 planes, their decode / hash statuses), the partial products of the reduction
// levels from pbase on, aggregate i at gbase + i (sigma_i: P1 planes, its running product: F planes, its status byte).  The sizes, the route
// and the scratch layout of a call are its plan (bn254_aggd_plan.h); aggd_device then runs:
//   1. aggd_front: decode the signatures (P2 planes at i), then k_aggd_prep: the aggregate's range checked, sigma_i and its status moved to
//      gbase + i, F = one there (an empty aggregate multiplies nothing into it); slot counts ceil(k_i / 2) for a device-side scan;
//   2. ... decode the keys, hash the messages (launch_decode_g2, launch_hash_rounds: the kernels and statuses of a verify);
//   3. ... k_aggd_map: per SLOT (two pairs of one aggregate) its aggregate by binary search of the scan; the first failing key / message
//      of every aggregate by atomicMin on the pair index;
//   4. aggd_levels: Miller loops and the segmented product (bn254_pair.hip): level 0 by the plan's route, then ceil(log_64) further levels;
//   5. k_aggd_status, then per aggregate F_i * miller(sigma_i, -G2) (the randomised verify's tail) and the final exponentiation of a verify
//      batch of n items, whose == one test gives 0 / 9 under the folded status.
// Against registered keys (bn254_batch_aggregate_verify_distinct_keyed[_device]): step 2 writes each pair's key status instead of decoding
// (k_aggd_keyed_keys), level 0 is the slot kernel of bn254_aggkeyed.hip over ALL k_i + 1 pairs of an aggregate, sigma's included (slots
// from a second count and scan: k_aggd_keyed_count / _map), and step 5 has no tail: the products move from gbase + i to i.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <cstring>

#include "../../include/bn254_hip.h"
#include "bn254_pairing.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"
#include "bn254_aggd_plan.h"

// ---- device-side scans over n aggregates (prefix maximum of the offsets, prefix sum of the slot counts) ---------------------------------
#define KERNEL_SCAN __global__ __launch_bounds__(AGGD_SCAN_WG)
struct AggdAdd { __device__ static uint64_t op(uint64_t a, uint64_t b) { return a + b; } };
struct AggdMax { __device__ static uint64_t op(uint64_t a, uint64_t b) { return a > b ? a : b; } };
// inclusive scan of one block of AGGD_SCAN_WG values in LDS (0 is the identity of both operations on unsigned values)
template <class Op>
__device__ __forceinline__ uint64_t aggd_block_scan(uint64_t v, uint64_t* lds) {
  const unsigned t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (unsigned d = 1; d < AGGD_SCAN_WG; d <<= 1) {
    const uint64_t o = t >= d ? lds[t - d] : 0;
    __syncthreads();
    v = Op::op(o, v);
    lds[t] = v;
    __syncthreads();
  }
  return v;
}
template <class Op>
KERNEL_SCAN void k_aggd_scan_block(const uint64_t* in, size_t n, uint64_t* out, uint64_t* tot) {
  __shared__ uint64_t lds[AGGD_SCAN_WG];
  const size_t i = (size_t)blockIdx.x * AGGD_SCAN_WG + threadIdx.x;
  const uint64_t v = aggd_block_scan<Op>(i < n ? in[i] : 0, lds);
  if (i < n) out[i] = v;
  if (threadIdx.x == AGGD_SCAN_WG - 1) tot[blockIdx.x] = v;
}
// one workgroup: the block totals scanned in place, AGGD_SCAN_WG at a time with a carry
template <class Op>
KERNEL_SCAN void k_aggd_scan_totals(uint64_t* tot, size_t nb) {
  __shared__ uint64_t lds[AGGD_SCAN_WG];
  uint64_t carry = 0;
  for (size_t b0 = 0; b0 < nb; b0 += AGGD_SCAN_WG) {
    const size_t b = b0 + threadIdx.x;
    const uint64_t v = Op::op(carry, aggd_block_scan<Op>(b < nb ? tot[b] : 0, lds));
    if (b < nb) tot[b] = v;
    carry = Op::op(carry, lds[AGGD_SCAN_WG - 1]);
    __syncthreads();
  }
}
template <class Op>
KERNEL_SCAN void k_aggd_scan_add(uint64_t* out, size_t n, const uint64_t* tot) {
  const size_t i = (size_t)blockIdx.x * AGGD_SCAN_WG + threadIdx.x;
  if (blockIdx.x > 0 && i < n) out[i] = Op::op(tot[blockIdx.x - 1], out[i]);
}
template <class Op>
static int aggd_scan(hipStream_t s, const uint64_t* in, size_t n, uint64_t* out, uint64_t* tot) {
  const size_t nb = (n + AGGD_SCAN_WG - 1) / AGGD_SCAN_WG;
  k_aggd_scan_block<Op><<<(unsigned)nb, AGGD_SCAN_WG, 0, s>>>(in, n, out, tot);
  if (nb > 1) {
    k_aggd_scan_totals<Op><<<1, AGGD_SCAN_WG, 0, s>>>(tot, nb);
    k_aggd_scan_add<Op><<<(unsigned)nb, AGGD_SCAN_WG, 0, s>>>(out, n, tot);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- bookkeeping kernels (one lane per aggregate / slot) ---------------------------------------------------------------------------------
// Aggregate i: its range [lo, hi) is accepted iff lo <= hi <= m and no earlier offset exceeds lo (mx = prefix maximum of the offsets) —
// the accepted ranges are then disjoint, so their slots fit the (m + n) / 2 the workspace holds.  Anything else: IndexOutOfBounds, no pairs.
KERNEL_SMALL void k_aggd_prep(size_t n, uint64_t m, const uint64_t* agg_off, const uint64_t* mx, uint64_t* cnt, uint64_t* lo_out, uint64_t* hi_out,
                              uint32_t* first_pk, uint32_t* first_hash, Ws ws, size_t gbase) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const uint64_t lo = agg_off[i], hi = agg_off[i + 1];
  const bool ok = lo <= hi && hi <= m && (i == 0 || mx[i - 1] <= lo);
  lo_out[i] = lo;
  hi_out[i] = ok ? hi : lo;
  cnt[i] = ok ? (hi - lo + 1) / 2 : 0;
  first_pk[i] = AGGD_SEG_NONE;
  first_hash[i] = AGGD_SEG_NONE;
  G1Affine sig;
  ws_load_g1(ws, PL_P2X, BY_P2_INF, i, sig);
  ws_store_g1(ws, PL_P1X, BY_P1_INF, gbase + i, sig);
  ws_byte(ws, BY_ST_DECODE, gbase + i) = ok ? ws_byte(ws, BY_ST_DECODE, i) : (uint8_t)ST_INDEX_OOB;
  Fp12 one;
  fp12_set_one(one);
  ws_store_f12(ws, gbase + i, one);
}
// slot e -> its aggregate (the first i whose inclusive slot count exceeds e; AGGD_SEG_NONE past the last slot) and its two pairs; the first
// failing key and the first failing message of the aggregate in pair order ("first non-zero in order" is a minimum over the pair index)
KERNEL_SMALL void k_aggd_map(size_t n_slots, size_t n, const uint64_t* incl, const uint64_t* lo, const uint64_t* hi, uint32_t* slot_agg,
                             uint32_t* pair_agg, uint32_t* first_pk, uint32_t* first_hash, Ws ws) {
  const size_t e = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (e >= n_slots) return;
  size_t a = 0, b = n;
  while (a < b) {
    const size_t mid = (a + b) >> 1;
    if (incl[mid] > e) b = mid; else a = mid + 1;
  }
  if (slot_agg) slot_agg[e] = a < n ? (uint32_t)a : AGGD_SEG_NONE;
  if (a >= n) return;
  const uint64_t l = lo[a], h = hi[a], j0 = l + 2 * (e - (incl[a] - (h - l + 1) / 2));
  for (uint64_t j = j0; j < j0 + 2 && j < h; ++j) {
    if (pair_agg) pair_agg[j] = (uint32_t)a;
    if (ws_byte(ws, BY_ST_DECODE, j) != ST_OK) atomicMin(&first_pk[a], (uint32_t)j);
    if (ws_byte(ws, BY_ST_HASH, j) != ST_OK) atomicMin(&first_hash[a], (uint32_t)j);
  }
}
// status of aggregate i: its range / signature status, else the first failing key's, else the first failing message's (then the pairing check)
KERNEL_SMALL void k_aggd_status(size_t n, Ws ws, size_t gbase, const uint32_t* first_pk, const uint32_t* first_hash) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  uint8_t st = ws_byte(ws, BY_ST_DECODE, gbase + i);
  if (st == ST_OK && first_pk[i] != AGGD_SEG_NONE) st = ws_byte(ws, BY_ST_DECODE, first_pk[i]);
  if (st == ST_OK && first_hash[i] != AGGD_SEG_NONE) st = ws_byte(ws, BY_ST_HASH, first_hash[i]);
  ws_byte(ws, BY_ST_DECODE, gbase + i) = st;
}

// ---- registered keys (bn254_batch_aggregate_verify_distinct_keyed) -----------------------------------------------------------------------
// pair j's key status in place of its decode status: 2 for an index >= n_keys, else what registration found (subgroup check included; the
// REJECT_IDENTITY of the registration).  expand = 1: the key itself into the Q planes at j (the generator for a refused key: its status is
// set, the arithmetic walks on), after which the pairs are those of the unkeyed call.  Never reads a table when nothing is registered.
KERNEL_SMALL void k_aggd_keyed_keys(size_t m, const uint32_t* key_idx, KeyTable kt, const int32_t* key_xy, Ws ws, int expand) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j >= m) return;
  const uint32_t key = key_idx[j];
  const bool in = key < kt.n_keys;
  const uint8_t kst = in ? kt.st[key] : (uint8_t)ST_INDEX_OOB;
  ws_byte(ws, BY_ST_DECODE, j) = kst;
  if (!expand) return;
  G2Affine q;
  if (kst == ST_OK) {
    const int32_t* w = key_xy + (size_t)key * 4 * BN_LIMBS;
    q.x.c0 = fp_load_const(w); q.x.c1 = fp_load_const(w + BN_LIMBS); q.y.c0 = fp_load_const(w + 2 * BN_LIMBS); q.y.c1 = fp_load_const(w + 3 * BN_LIMBS);
    q.inf = kt.inf[key] != 0;
  } else {
    g2_set_generator(q);
  }
  ws_store_g2(ws, j, q);
}
// slots of the slot kernel per aggregate: its k + 1 table pairs (sigma's included), `width` per slot
KERNEL_SMALL void k_aggd_keyed_count(size_t n, const uint64_t* lo, const uint64_t* hi, uint64_t width, uint64_t* cnt) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  cnt[i] = (hi[i] - lo[i] + width) / width;
}
// slot e -> its aggregate: the first i whose inclusive slot count exceeds e (AGGD_SEG_NONE past the last slot)
KERNEL_SMALL void k_aggd_keyed_map(size_t n_slots, size_t n, const uint64_t* incl, uint32_t* slot_agg) {
  const size_t e = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (e >= n_slots) return;
  size_t a = 0, b = n;
  while (a < b) {
    const size_t mid = (a + b) >> 1;
    if (incl[mid] > e) b = mid; else a = mid + 1;
  }
  slot_agg[e] = a < n ? (uint32_t)a : AGGD_SEG_NONE;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// a call's arguments as device pointers; keyed: pk_j = the registered key d_key_idx[j] and d_pks is null, else the other way round
struct AggdArgs {
  const uint8_t* d_msgs; const uint64_t* d_msg_off; const uint8_t* d_pks; const uint32_t* d_key_idx; bool keyed; size_t m;
  const uint8_t* d_sigs; const uint64_t* d_agg_off; size_t n; uint32_t flags; uint8_t* d_status;
};
// Steps 1-3 of every route.  width: table pairs per slot of the slot kernel (its slots' aggregates into kslot_agg), 0 without it — then a
// keyed call expands its keys into the Q planes; slot_agg / pair_agg: k_aggd_map's outputs a route reads (pairs outside every accepted
// range belong to nobody), else null.  No pairs: nothing past the scans.
static int aggd_front(bn254_ctx* c, hipStream_t s, const AggdArgs& a, const KeyTable& kt, const AggdFrontBufs& f, size_t gbase, size_t n_slots, int width,
                      size_t n_kslots, uint32_t* slot_agg, uint32_t* pair_agg, uint32_t* kslot_agg) {
  const uint32_t dflags = a.flags & (BN254_FLAG_G2_SUBGROUP_CHECK | BN254_FLAG_REJECT_IDENTITY);
  const size_t m = a.m, n = a.n;
  int rc;
  if ((rc = launch_decode_g1(c, s, a.d_sigs, n, dflags, PL_P2X, BY_P2_INF, 0))) return rc;
  if ((rc = aggd_scan<AggdMax>(s, a.d_agg_off, n, f.mx, f.tot))) return rc;
  k_aggd_prep<<<grid_for(n), BN_WAVE, 0, s>>>(n, (uint64_t)m, a.d_agg_off, f.mx, f.incl, f.lo, f.hi, f.first_pk, f.first_hash, c->ws, gbase);
  if ((rc = aggd_scan<AggdAdd>(s, f.incl, n, f.incl, f.tot))) return rc;
  if (width) {
    k_aggd_keyed_count<<<grid_for(n), BN_WAVE, 0, s>>>(n, f.lo, f.hi, (uint64_t)width, f.kincl);
    if ((rc = aggd_scan<AggdAdd>(s, f.kincl, n, f.kincl, f.tot))) return rc;
  }
  if (!m) { PROF_MARK(1); PROF_MARK(2); return 0; }
  if (a.keyed) {
    k_aggd_keyed_keys<<<grid_for(m), BN_WAVE, 0, s>>>(m, a.d_key_idx, kt, c->key_xy, c->ws, width ? 0 : 1);
    HIP_TRY(hipGetLastError());
  } else if ((rc = launch_decode_g2(c, s, a.d_pks, m, dflags, 0))) {
    return rc;
  }
  PROF_MARK(1);
  if ((rc = launch_hash_rounds(c, s, a.d_msgs, a.d_msg_off, m, PL_P1X, BY_P1_INF, nullptr))) return rc;
  PROF_MARK(2);
  if (pair_agg) HIP_TRY(hipMemsetAsync(pair_agg, 0xFF, 4 * m, s));
  k_aggd_map<<<grid_for(n_slots), BN_WAVE, 0, s>>>(n_slots, n, f.incl, f.lo, f.hi, slot_agg, pair_agg, f.first_pk, f.first_hash, c->ws);
  if (width) k_aggd_keyed_map<<<grid_for(n_kslots), BN_WAVE, 0, s>>>(n_kslots, n, f.kincl, kslot_agg);
  return 0;
}
// level 0 of a segmented Fq12 product over e0 elements (level0(e, pbase, pseg, last): Miller loops and, on lane pairs, the first product;
// only it writes at entry 0), then the level kernel over the partials the level before left at `in`; nothing is launched after an error
template <class Level0>
static int aggd_levels(bn254_ctx* c, hipStream_t s, size_t e0, size_t gbase, size_t pbase, uint32_t* pseg, Level0 level0) {
  int rc = 0;
  size_t in = 0;
  seg_levels(e0, AGGD_WG_ELEMS, [&](size_t e, size_t off, int last) {
    if (!rc) rc = !off ? level0(e, pbase, pseg, last) : bn254_pair_aggd_level(e, c->ws, pseg + in, pbase + in, gbase, pbase + off, pseg + off, last, s);
    in = off;
  });
  return rc;
}

// the exact calls: plan -> reserve -> steps 1-3 -> levels -> status -> tail / move -> final exponentiation
static int aggd_device(bn254_ctx* c, const AggdArgs& a, hipStream_t s) {
  const size_t m = a.m, n = a.n;
  const bool lane_machine = c->pair_lanes && route_lane_machine_helpers(c, m);
  const bool have_keys = c->n_keys > 0 && c->key_lines;
  const AggdPlan p = aggd_plan(m, n, a.keyed, have_keys, c->pair_lanes, lane_machine, c->aggd_keyed_route);
  Carve size(nullptr);                                 // the layout run twice: on a null base for the byte count, then on the buffer
  aggd_scratch(size, p);
  int rc = ws_reserve(c, p.ws_items);
  if (rc || (rc = scratch_reserve(c, &c->aggd_buf, &c->aggd_cap, size.used))) return rc;
  Carve carve(c->aggd_buf);
  const AggdScratch b = aggd_scratch(carve, p);
  const KeyTable kt = {c->key_lines, c->key_st, c->key_inf, (uint32_t)(have_keys ? c->n_keys : 0)};
  CallDone call_done(c, s);
  PROF_MARK(0);
  if ((rc = aggd_front(c, s, a, kt, b.f, p.gbase, p.n_slots, p.width, p.n_kslots, p.route == AGGD_TWO_PER_PAIR ? b.seg0 : nullptr,
                       p.route == AGGD_PER_PAIR ? b.seg0 : nullptr, p.route == AGGD_SLOTS ? b.seg0 : nullptr)))
    return rc;
  if (m) {
    const AggdSlots sl = {b.seg0, p.route == AGGD_SLOTS ? b.f.kincl : b.f.incl, b.f.lo, b.f.hi};
    rc = aggd_levels(c, s, p.e0, p.gbase, p.pbase, b.pseg, [&](size_t e, size_t pb, uint32_t* ps, int last) -> int {
      int r;
      if (p.route == AGGD_SLOTS) r = bn254_pair_aggd_keyed(e, p.width, c->ws, sl, a.d_key_idx, kt, p.gbase, pb, ps, last, s);
      else if (p.route == AGGD_TWO_PER_PAIR) r = bn254_pair_aggd_miller(e, c->ws, sl, p.gbase, pb, ps, last, s);
      else if (lane_machine) r = bn254_lm_miller_verify(m, c->ws, s, 2);      // a single pair e(P1, Q) per lane-machine verify
      else if (c->pair_lanes) r = bn254_pair_miller_var(m, c->ws, s);
      else r = launch_miller_var_lane(c, s, m);
      if (r) return r;
      PROF_MARK(3);
      return p.route == AGGD_PER_PAIR ? bn254_pair_aggd_level(e, c->ws, b.seg0, 0, p.gbase, pb, ps, last, s) : 0;   // ... then the product over the pairs
    });
    if (rc) return rc;
  } else PROF_MARK(3);
  k_aggd_status<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws, p.gbase, b.f.first_pk, b.f.first_hash);
  if (c->pair_lanes) {
    // into index i: with sigma's pair already in every product (slot kernel) F and the status move; else the tail (obase 0: everything below
    // gbase is consumed by now).  Then the final exponentiation a verify of n items runs.
    if ((rc = p.route == AGGD_SLOTS ? bn254_pair_aggd_move(n, c->ws, p.gbase, s) : bn254_pair_aggd_tail(n, c->ws, p.gbase, 0, s))) return rc;
    if ((rc = launch_final_exp_layout(c, s, n, 0, a.d_status, route_for(c, n).fe))) return rc;
  } else {
    if ((rc = launch_rand_tail_lane(c, s, n, p.gbase))) return rc;
    if ((rc = launch_final_exp_lane(c, s, n, 1, 1, 1, 0, nullptr, a.d_status, 0, p.gbase, nullptr, nullptr))) return rc;
  }
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- registered keys, randomised (bn254_batch_aggregate_verify_distinct_keyed_randomized[_device]; kernels: bn254_aggrand.hip) -------------
// Steps 1-3 (aggd_front, with each pair's aggregate for the G1 side) and the status fold are the exact keyed call's; then the G1 side (scaled
// entries, buckets by (group, key), their segmented sums), ONE slot-kernel check per group over its table pairs (a bucket's sum and its key;
// S_g and -G2), the collect, and the exact slot kernel for the aggregates of failed groups only.  Workspace (AggrPlan): H(m_j) stays in
// the P1 planes at j and sigma_i at gbase + i throughout; the scaled entries r_i H(m_j), r_i sigma_i go to P2 / HASHX at the same index.
static int aggr_device(bn254_ctx* c, const AggdArgs& a, const uint8_t* seed32, hipStream_t s) {
  const size_t m = a.m, n = a.n, K = c->n_keys;
  const AggrPlan p = aggr_plan(m, n, K, (size_t)c->agg_rand_group_pairs, c->aggd_keyed_route);
  Carve size(nullptr);
  aggr_scratch(size, p);
  int rc = ws_reserve(c, p.ws_items);
  if (rc || (rc = scratch_reserve(c, &c->aggr_buf, &c->aggr_cap, size.used))) return rc;
  Carve carve(c->aggr_buf);
  const AggrScratch b = aggr_scratch(carve, p);
  if (!c->aggr_stats) HIP_TRY(hipMalloc((void**)&c->aggr_stats, 8 * sizeof(uint32_t)));
  const KeyTable kt = {c->key_lines, c->key_st, c->key_inf, (uint32_t)K};
  uint32_t seed_w[8];
  for (int j = 0; j < 8; ++j)
    seed_w[j] = ((uint32_t)seed32[4 * j] << 24) | ((uint32_t)seed32[4 * j + 1] << 16) | ((uint32_t)seed32[4 * j + 2] << 8) | seed32[4 * j + 3];
  const int mode = (a.flags & BN254_FLAG_RAND64) ? 1 : (a.flags & BN254_FLAG_RAND_GLV) ? 2 : 0;
  CallDone call_done(c, s);
  c->aggr_last = {p.ng, p.cbase, p.tbase, b.nagg, b.bkey, b.glo, b.ghi, b.gst};   // nothing below rewrites these once the group checks are through
  PROF_MARK(0);
  if ((rc = aggd_front(c, s, a, kt, b.f, p.gbase, p.n_slots, p.wx, p.n_xslots, nullptr, b.pair_agg, b.xseg0))) return rc;
  k_aggd_status<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws, p.gbase, b.f.first_pk, b.f.first_hash);
  // the G1 side: scaled entries counted by bucket, sorted, summed into the groups' table pairs and S_g
  HIP_TRY(hipMemsetAsync(b.nagg, 0, 4 * p.ng, s));
  HIP_TRY(hipMemsetAsync(b.cnt, 0, 8 * p.n_b, s));
  HIP_TRY(hipMemsetAsync(b.eseg, 0xFF, 4 * p.n_e, s));
  const AggrScale sc = {b.pair_agg, a.d_key_idx, c->key_inf, b.f.lo, b.nagg, b.ebkt, b.cnt, (uint64_t)p.G, (uint32_t)K};
  if ((rc = bn254_aggr_scale(m, n, c->ws, p.gbase, sc, seed_w, mode, s))) return rc;
  if ((rc = aggd_scan<AggdAdd>(s, b.cnt, p.n_b, b.tp, b.f.tot))) return rc;
  if ((rc = bn254_aggr_scatter(p.n_e, b.ebkt, b.tp, b.perm, b.eseg, p.n_b, (uint32_t)K, b.cnt, b.tp, s))) return rc;
  if ((rc = aggd_scan<AggdAdd>(s, b.tp, p.n_b, b.tp, b.f.tot))) return rc;
  if ((rc = bn254_aggr_glimits(p.ng, (uint32_t)K, p.tbase, b.cnt, b.tp, b.glo, b.ghi, c->ws, p.cbase, s))) return rc;
  const AggrSum sm = {b.perm, b.tp, b.bkey, m, p.gbase, p.cbase, p.tbase, (uint32_t)K};
  size_t in = 0;                                       // the levels of the sums, as aggd_levels: level 0 reads the sorted entries
  seg_levels(p.n_e, AGGR_SUM_WG, [&](size_t e, size_t off, int last) {
    if (!rc) rc = bn254_aggr_sum(e, !off, c->ws, sm, off ? b.spseg + in : b.eseg, off ? b.part + AGGR_PART_WORDS * in : nullptr, b.spseg + off,
                                 b.part + AGGR_PART_WORDS * off, last, s);
    in = off;
  });
  if (rc) return rc;
  PROF_MARK(3);                                        // ms[2] = hash .. sums, ms[3] = group checks, collect and re-check
  // one check per group: its table pairs and (S_g, -G2) through the slot kernel, the levels, the final exponentiation at index g
  k_aggd_keyed_count<<<grid_for(p.ng), BN_WAVE, 0, s>>>(p.ng, b.glo, b.ghi, (uint64_t)p.wg, b.gkincl);
  if ((rc = aggd_scan<AggdAdd>(s, b.gkincl, p.ng, b.gkincl, b.f.tot))) return rc;
  k_aggd_keyed_map<<<grid_for(p.n_gslots), BN_WAVE, 0, s>>>(p.n_gslots, p.ng, b.gkincl, b.gseg0);
  const AggdSlots gsl = {b.gseg0, b.gkincl, b.glo, b.ghi};
  if ((rc = aggd_levels(c, s, p.n_gslots, p.cbase, p.pbase, b.pseg, [&](size_t e, size_t pb, uint32_t* ps, int last) {
         return bn254_pair_aggd_keyed_queued(e, p.wg, c->ws, gsl, b.bkey, kt, p.cbase, pb, ps, last, nullptr, s);   // empty workgroups leave
       })))
    return rc;
  if ((rc = bn254_pair_aggd_move(p.ng, c->ws, p.cbase, s))) return rc;
  if ((rc = launch_final_exp_layout(c, s, p.ng, 0, b.gst, route_for(c, p.ng).fe))) return rc;
  // statuses; the aggregates of failed groups (of two or more) queued and checked exactly — with none queued, launches that leave at once
  HIP_TRY(hipMemsetAsync(c->ws.h_cnt, 0, sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(c->aggr_stats, 0, 8 * sizeof(uint32_t), s));
  if ((rc = bn254_aggr_collect(n, c->ws, p.gbase, b.f.lo, (uint64_t)p.G, b.nagg, b.gst, a.d_status, b.queued, p.ng, b.glo, b.ghi, c->aggr_stats, s))) return rc;
  const AggdSlots xsl = {b.xseg0, b.f.kincl, b.f.lo, b.f.hi};
  if ((rc = aggd_levels(c, s, p.n_xslots, p.gbase, p.pbase, b.pseg, [&](size_t e, size_t pb, uint32_t* ps, int last) {
         return bn254_pair_aggd_keyed_queued(e, p.wx, c->ws, xsl, a.d_key_idx, kt, p.gbase, pb, ps, last, b.queued, s);
       })))
    return rc;
  if ((rc = bn254_pair_aggd_move(n, c->ws, p.gbase, s))) return rc;
  if ((rc = bn254_pair_final_exp(n, c->ws, 0, a.d_status, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  c->aggr_last_ran = 1;                                // only a call that enqueued everything has something for the debug hooks to read
  return 0;
}

// ---- the six entry points (include/bn254_hip.h) over two helpers ----------------------------------------------------------------------------
enum AggdCall { AGGD_UNKEYED, AGGD_KEYED, AGGD_RANDOMIZED };
// the *_device forms: argument checks (bad argument before misaligned), then the call on `stream` or the context's own
static int aggd_call_device(bn254_ctx* c, AggdCall call, const AggdArgs& a, const uint8_t* seed32, void* stream) {
  MsgsLenScope msgs_len_scope(c);
  const void* third = a.keyed ? (const void*)a.d_key_idx : a.d_pks;
  if (!c || g1c_flag(a.flags) || (call == AGGD_RANDOMIZED && !seed32) || !a.d_agg_off || (a.n && (!a.d_sigs || !a.d_status)) || (a.m && (!a.d_msgs || !a.d_msg_off || !third)))
    return BN254_E_BAD_ARGUMENT;
  if (a.m > 0xFFFFFFFFu || a.n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (call == AGGD_RANDOMIZED) c->aggr_last_ran = 0;
  if (a.n == 0) return 0;
  if (misaligned(a.d_sigs) || misaligned(third) || ((uintptr_t)a.d_msg_off & 7u) || ((uintptr_t)a.d_agg_off & 7u)) return BN254_E_MISALIGNED;
  // no keys, pair lanes off, too few messages (or none): the exact keyed call, same bytes; entries are numbered in 32 bits
  const bool exact = call != AGGD_RANDOMIZED || c->n_keys == 0 || !c->key_lines || !c->pair_lanes || a.m == 0 || a.m < (size_t)c->agg_rand_min_pairs ||
                     a.m + a.n > 0xFFFFFFFFu;
  HIP_TRY(hipSetDevice(c->device));
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return exact ? aggd_device(c, a, s) : aggr_device(c, a, seed32, s);
}
// the host-pointer forms: the offsets checked where the host can see them, the arrays staged (the third one: m entries of third_size
// bytes — keys of 128, key indices of 4), the *_device form on the context's stream, the statuses copied back
static int aggd_call_host(bn254_ctx* c, AggdCall call, const uint8_t* msgs, const uint64_t* msg_off, const void* third, size_t third_size, size_t m,
                          const uint8_t* agg_sigs, const uint64_t* agg_off, size_t n, uint32_t flags, const uint8_t* seed32, uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || g1c_flag(flags) || (call == AGGD_RANDOMIZED && !seed32) || !msg_off || !agg_off || (n && (!agg_sigs || !status)) || (m && !third)) return BN254_E_BAD_ARGUMENT;
  if (m > 0xFFFFFFFFu || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (agg_off[0] != 0 || agg_off[n] != m || !offsets_ok(agg_off, n) || !offsets_ok(msg_off, m)) return BN254_E_BAD_ARGUMENT;
  if (call == AGGD_RANDOMIZED) c->aggr_last_ran = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, msg_off, m)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)msg_off[m]), *d_msg_off = st.in(1, msg_off, (m + 1) * sizeof(uint64_t));
  const uint8_t *d_third = st.in(2, third, m * third_size), *d_agg_sigs = st.in(3, agg_sigs, n * 64), *d_agg_off = st.in(4, agg_off, (n + 1) * sizeof(uint64_t));
  uint8_t* d_status = st.out(5, n, status);
  const bool keyed = call != AGGD_UNKEYED;
  if (st.ok())
    st.rc = aggd_call_device(c, call, {d_msgs, (const uint64_t*)d_msg_off, keyed ? nullptr : d_third, keyed ? (const uint32_t*)d_third : nullptr, keyed, m,
                                       d_agg_sigs, (const uint64_t*)d_agg_off, n, flags, d_status}, seed32, nullptr);
  return st.finish();
}

extern "C" {
int bn254_batch_aggregate_verify_distinct_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_pks, size_t m,
                                                 const uint8_t* d_agg_sigs, const uint64_t* d_agg_off, size_t n, uint32_t flags, uint8_t* d_status,
                                                 void* stream) {
  return aggd_call_device(c, AGGD_UNKEYED, {d_msgs, d_msg_off, d_pks, nullptr, false, m, d_agg_sigs, d_agg_off, n, flags, d_status}, nullptr, stream);
}
int bn254_batch_aggregate_verify_distinct(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pks, size_t m, const uint8_t* agg_sigs,
                                          const uint64_t* agg_off, size_t n, uint32_t flags, uint8_t* status) {
  return aggd_call_host(c, AGGD_UNKEYED, msgs, msg_off, pks, 128, m, agg_sigs, agg_off, n, flags, nullptr, status);
}
int bn254_batch_aggregate_verify_distinct_keyed_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint32_t* d_key_idx, size_t m,
                                                       const uint8_t* d_agg_sigs, const uint64_t* d_agg_off, size_t n, uint32_t flags, uint8_t* d_status,
                                                       void* stream) {
  return aggd_call_device(c, AGGD_KEYED, {d_msgs, d_msg_off, nullptr, d_key_idx, true, m, d_agg_sigs, d_agg_off, n, flags, d_status}, nullptr, stream);
}
int bn254_batch_aggregate_verify_distinct_keyed(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* key_idx, size_t m,
                                                const uint8_t* agg_sigs, const uint64_t* agg_off, size_t n, uint32_t flags, uint8_t* status) {
  return aggd_call_host(c, AGGD_KEYED, msgs, msg_off, key_idx, sizeof(uint32_t), m, agg_sigs, agg_off, n, flags, nullptr, status);
}
int bn254_batch_aggregate_verify_distinct_keyed_randomized_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint32_t* d_key_idx,
                                                                  size_t m, const uint8_t* d_agg_sigs, const uint64_t* d_agg_off, size_t n, uint32_t flags,
                                                                  const uint8_t* seed32, uint8_t* d_status, void* stream) {
  return aggd_call_device(c, AGGD_RANDOMIZED, {d_msgs, d_msg_off, nullptr, d_key_idx, true, m, d_agg_sigs, d_agg_off, n, flags, d_status}, seed32, stream);
}
int bn254_batch_aggregate_verify_distinct_keyed_randomized(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* key_idx, size_t m,
                                                           const uint8_t* agg_sigs, const uint64_t* agg_off, size_t n, uint32_t flags, const uint8_t* seed32,
                                                           uint8_t* status) {
  return aggd_call_host(c, AGGD_RANDOMIZED, msgs, msg_off, key_idx, sizeof(uint32_t), m, agg_sigs, agg_off, n, flags, seed32, status);
}
}  // extern "C"

// for the other unit that runs group checks (bn254_bitmap_rand.hip): the prefix sum, and the slot kernel's slots of n groups of table pairs
int bn254_aggd_scan_add(hipStream_t s, const uint64_t* in, size_t n, uint64_t* out, uint64_t* tot) { return aggd_scan<AggdAdd>(s, in, n, out, tot); }
int bn254_aggd_scan_max(hipStream_t s, const uint64_t* in, size_t n, uint64_t* out, uint64_t* tot) { return aggd_scan<AggdMax>(s, in, n, out, tot); }
int bn254_aggd_keyed_slot_map(hipStream_t s, size_t n, const uint64_t* lo, const uint64_t* hi, int width, uint64_t* kincl, uint64_t* tot, size_t n_slots,
                              uint32_t* slot_agg) {
  k_aggd_keyed_count<<<grid_for(n), BN_WAVE, 0, s>>>(n, lo, hi, (uint64_t)width, kincl);
  if (const int rc = aggd_scan<AggdAdd>(s, kincl, n, kincl, tot)) return rc;
  k_aggd_keyed_map<<<grid_for(n_slots), BN_WAVE, 0, s>>>(n_slots, n, kincl, slot_agg);
  HIP_TRY(hipGetLastError());
  return 0;
}
