// Translation unit of libbn254hip.so: aggregate verification over DISTINCT messages (include/bn254_hip.h:
// bn254_batch_aggregate_verify_distinct[_device]) — the host side and the one-lane bookkeeping kernels.  Aggregate i owns the pairs
// j in [agg_off[i], agg_off[i+1]) and passes iff  e(sigma_i, -G2::one()) * prod_j e(H(m_j), pk_j) == 1  (the IRTF draft's AggregateVerify;
// the sums are the reference's `Add for Signature`, src/types.rs:264-270; the check is ECDSA::verify's, src/ecdsa.rs:49-64).
//
// Workspace: pair j at index j (key: Q planes, H(m_j): P1 planes, their decode / hash statuses), the partial products of the reduction
// levels from pbase on, aggregate i at gbase + i (sigma_i: P1 planes, its running product: F planes, its status byte).  Steps:
//   1. decode the signatures (P2 planes at i), then k_aggd_prep: the aggregate's range checked, sigma_i and its status moved to gbase + i,
//      F = one there (an empty aggregate multiplies nothing into it); slot counts ceil(k_i / 2) for a device-side scan;
//   2. decode the keys, hash the messages (launch_decode_g2, launch_hash_rounds: the kernels and statuses of a verify);
//   3. k_aggd_map: per SLOT (two pairs of one aggregate) its aggregate by binary search of the scan; the first failing key / message of
//      every aggregate by atomicMin on the pair index;
//   4. Miller loops and the segmented product (bn254_pair.hip): level 0, then ceil(log_64) further levels over the partials — level 0 is
//      the segmented Miller kernel (two pairs per lane pair) from AGGD_TWO_PER_PAIR_MIN_M pairs on, below that one Miller loop per pair
//      (lane machine for the smallest m, lane pairs, or one lane with pair_lanes off) followed by the level kernel over the pairs;
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

// ---- device-side scans over n aggregates (prefix maximum of the offsets, prefix sum of the slot counts) ---------------------------------
#define AGGD_SCAN_WG 256
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
static inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
// entries of the partial array all levels need: a level of e elements runs ceil(e / 128) workgroups and, unless that is one, leaves two each
static size_t aggd_partials(size_t e) {
  size_t p = 0;
  for (;;) {
    const size_t g = (e + AGGD_WG_ELEMS - 1) / AGGD_WG_ELEMS;
    if (g <= 1) return p;
    p += 2 * g;
    e = 2 * g;
  }
}
static int aggd_reserve(bn254_ctx* c, size_t bytes) {
  if (bytes <= c->aggd_cap) return 0;
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  if (c->aggd_buf) { HIP_TRY(hipFree(c->aggd_buf)); c->aggd_buf = nullptr; c->aggd_cap = 0; }
  const size_t cap = (bytes + 4095) & ~(size_t)4095;
  HIP_TRY(hipMalloc((void**)&c->aggd_buf, cap));
  c->aggd_cap = cap;
  return 0;
}

// keyed: bn254_batch_aggregate_verify_distinct_keyed — pk_j = the registered key d_key_idx[j], d_pks unused
static int aggd_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_pks, bool keyed, const uint32_t* d_key_idx, size_t m,
                       const uint8_t* d_sigs, const uint64_t* d_agg_off, size_t n, uint32_t flags, uint8_t* d_status, hipStream_t s) {
  const uint32_t dflags = flags & (BN254_FLAG_G2_SUBGROUP_CHECK | BN254_FLAG_REJECT_IDENTITY);
  // routes: small m -> one pairing per lane-machine verify (latency); pair_lanes off -> one pairing per lane; m below AGGD_TWO_PER_PAIR_MIN_M ->
  // one pair per lane pair (fills the chip); else two pairs of an aggregate per lane pair, the first product fused into the Miller kernel
  const bool lane_machine = c->pair_lanes && route_lane_machine_helpers(c, m);
  // keyed: the slot kernel on the registered tables (sigma's pair in a slot like any other: no tail) at every size — it beats the expanded
  // keys on the lane machine too, whose sigma tail is a whole Miller loop.  One table pair per lane pair while those fit
  // one pass of two waves per SIMD, else two.  pair_lanes off and an empty key set expand the keys into the Q planes and run the unkeyed
  // route from the map on.
  const bool have_keys = c->n_keys > 0 && c->key_lines;
  const int kr = c->aggd_keyed_route;
  const bool slots = keyed && m && c->pair_lanes && have_keys && kr != 3;
  const int width = !slots ? 0 : kr ? kr : m + n <= AGGD_KEYED_W1_MAX_SLOTS ? 1 : 2;
  const bool per_pair = !slots && (lane_machine || !c->pair_lanes || m < AGGD_TWO_PER_PAIR_MIN_M);
  const size_t n_slots = (m + n + 1) / 2;             // sum of ceil(k_i / 2) over disjoint ranges
  const size_t n_kslots = width == 1 ? m + n : m / 2 + n;   // sum of ceil((k_i + 1) / width)
  const size_t e0 = slots ? n_kslots : per_pair ? m : n_slots;
  const size_t n_part = m ? aggd_partials(e0) : 0;
  const size_t pbase = round256(m), gbase = round256(pbase + n_part > n ? pbase + n_part : n);
  int rc = ws_reserve(c, gbase + n);
  if (rc) return rc;
  const size_t nb = (n + AGGD_SCAN_WG - 1) / AGGD_SCAN_WG;
  const size_t n_seg0 = e0;
  const size_t u64_words = (slots ? 5 : 4) * n + nb, u32_words = 2 * n + n_seg0 + n_part;
  if ((rc = aggd_reserve(c, 8 * u64_words + 4 * u32_words))) return rc;
  uint64_t* mx = (uint64_t*)c->aggd_buf;
  uint64_t* incl = mx + n;
  uint64_t* lo = incl + n;
  uint64_t* hi = lo + n;
  uint64_t* tot = hi + n;
  uint64_t* kincl = tot + nb;                                            // keyed slots: the inclusive scan of the slot counts
  uint32_t* first_pk = (uint32_t*)(kincl + (slots ? n : 0));
  uint32_t* first_hash = first_pk + n;
  uint32_t* seg0 = first_hash + n;
  uint32_t* pseg = seg0 + n_seg0;
  const KeyTable kt = {c->key_lines, c->key_st, c->key_inf, (uint32_t)(have_keys ? c->n_keys : 0)};
  CallDone call_done(c, s);
  PROF_MARK(0);
  if ((rc = launch_decode_g1(c, s, d_sigs, n, dflags, PL_P2X, BY_P2_INF, 0))) return rc;
  if ((rc = aggd_scan<AggdMax>(s, d_agg_off, n, mx, tot))) return rc;
  k_aggd_prep<<<grid_for(n), BN_WAVE, 0, s>>>(n, (uint64_t)m, d_agg_off, mx, incl, lo, hi, first_pk, first_hash, c->ws, gbase);
  if ((rc = aggd_scan<AggdAdd>(s, incl, n, incl, tot))) return rc;
  if (slots) {
    k_aggd_keyed_count<<<grid_for(n), BN_WAVE, 0, s>>>(n, lo, hi, (uint64_t)width, kincl);
    if ((rc = aggd_scan<AggdAdd>(s, kincl, n, kincl, tot))) return rc;
  }
  if (m) {
    if (keyed) {
      k_aggd_keyed_keys<<<grid_for(m), BN_WAVE, 0, s>>>(m, d_key_idx, kt, c->key_xy, c->ws, slots ? 0 : 1);
      HIP_TRY(hipGetLastError());
    } else if ((rc = launch_decode_g2(c, s, d_pks, m, dflags, 0))) {
      return rc;
    }
    PROF_MARK(1);
    if ((rc = launch_hash_rounds(c, s, d_msgs, d_msg_off, m, PL_P1X, BY_P1_INF, nullptr))) return rc;
    PROF_MARK(2);
    if (per_pair) HIP_TRY(hipMemsetAsync(seg0, 0xFF, 4 * m, s));          // pairs outside every accepted range belong to nobody
    const bool two = !per_pair && !slots;                                  // the unkeyed segmented two-pair Miller kernel
    k_aggd_map<<<grid_for(n_slots), BN_WAVE, 0, s>>>(n_slots, n, incl, lo, hi, two ? seg0 : nullptr, per_pair ? seg0 : nullptr, first_pk, first_hash,
                                                       c->ws);
    if (slots) k_aggd_keyed_map<<<grid_for(n_kslots), BN_WAVE, 0, s>>>(n_kslots, n, kincl, seg0);
    // level 0 (Miller loops, and on lane pairs the first product), then the levels over the partials until one workgroup holds them all
    size_t e = e0, ebase = 0, off = 0;
    const uint32_t* seg = seg0;
    bool level0 = true;
    for (;;) {
      const size_t g = (e + AGGD_WG_ELEMS - 1) / AGGD_WG_ELEMS;
      const int last = g <= 1;
      if (level0 && slots) {
        const AggdSlots sl = {seg0, kincl, lo, hi};
        if ((rc = bn254_pair_aggd_keyed(e, width, c->ws, sl, d_key_idx, kt, gbase, pbase + off, pseg + off, last, s))) return rc;
        PROF_MARK(3);
      } else if (level0 && !per_pair) {
        const AggdSlots sl = {seg0, incl, lo, hi};
        if ((rc = bn254_pair_aggd_miller(e, c->ws, sl, gbase, pbase + off, pseg + off, last, s))) return rc;
        PROF_MARK(3);
      } else {
        if (level0) {
          if (lane_machine) rc = bn254_lm_miller_verify(m, c->ws, s, 2);    // a single pair e(P1, Q) per lane-machine verify
          else if (c->pair_lanes) rc = bn254_pair_miller_var(m, c->ws, s);
          else rc = launch_miller_var_lane(c, s, m);
          if (rc) return rc;
          PROF_MARK(3);
        }
        if ((rc = bn254_pair_aggd_level(e, c->ws, seg, ebase, gbase, pbase + off, pseg + off, last, s))) return rc;
      }
      level0 = false;
      if (last) break;
      e = 2 * g;
      ebase = pbase + off;
      seg = pseg + off;
      off += 2 * g;
    }
  } else {
    PROF_MARK(1);
    PROF_MARK(2);
    PROF_MARK(3);
  }
  k_aggd_status<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws, gbase, first_pk, first_hash);
  if (slots) {
    // sigma's pair is already in every product: move F and the status to index i, then the final exponentiation a verify of n items runs
    if ((rc = bn254_pair_aggd_move(n, c->ws, gbase, s))) return rc;
    if ((rc = launch_final_exp_layout(c, s, n, 0, d_status, route_for(c, n).fe))) return rc;
  } else if (c->pair_lanes) {
    // tail into index i (obase 0: everything below gbase is consumed by now), then the final exponentiation a verify of n items runs
    if ((rc = bn254_pair_aggd_tail(n, c->ws, gbase, 0, s))) return rc;
    if ((rc = launch_final_exp_layout(c, s, n, 0, d_status, route_for(c, n).fe))) return rc;
  } else {
    if ((rc = launch_rand_tail_lane(c, s, n, gbase))) return rc;
    if ((rc = launch_final_exp_lane(c, s, n, 1, 1, 1, 0, nullptr, d_status, 0, gbase, nullptr, nullptr))) return rc;
  }
  PROF_MARK(4);
  if (c->profiling) { c->ev_valid = 1; c->ev_hash_first = 0; }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- registered keys, randomised (bn254_batch_aggregate_verify_distinct_keyed_randomized[_device]; kernels: bn254_aggrand.hip) -------------
// Steps 1-3 and the status fold are the exact keyed call's; then the G1 side (scaled entries, buckets by (group, key), their segmented sums),
// ONE slot-kernel check per group over its table pairs (a bucket's sum and its key; S_g and -G2), the collect, and the exact slot kernel
// for the aggregates of failed groups only.  Workspace: pairs at j (H(m_j) in the P1 planes throughout; scaled entries in P2 / HASHX),
// the Fq12 partials of both checks from pbase, aggregates from gbase (sigma_i in P1, r_i sigma_i in P2 / HASHX), groups from cbase (S_g,
// their products), the groups' table pairs from tbase.
static size_t aggr_partials(size_t e) {
  size_t p = 0;
  for (;;) {
    const size_t g = (e + AGGR_SUM_WG - 1) / AGGR_SUM_WG;
    if (g <= 1) return p;
    p += 2 * g;
    e = 2 * g;
  }
}
// level 0 of a segmented Fq12 product over e0 slot elements (level0(e, pbase, pseg, last)), then the level kernel until one workgroup is left
template <class Level0>
static int aggd_levels(bn254_ctx* c, hipStream_t s, size_t e0, size_t gbase, size_t pbase, uint32_t* pseg, Level0 level0) {
  size_t e = e0, ebase = 0, off = 0;
  const uint32_t* seg = nullptr;
  for (bool first = true;; first = false) {
    const size_t g = (e + AGGD_WG_ELEMS - 1) / AGGD_WG_ELEMS;
    const int last = g <= 1;
    if (const int rc = first ? level0(e, pbase + off, pseg + off, last) : bn254_pair_aggd_level(e, c->ws, seg, ebase, gbase, pbase + off, pseg + off, last, s))
      return rc;
    if (last) return 0;
    e = 2 * g;
    ebase = pbase + off;
    seg = pseg + off;
    off += 2 * g;
  }
}
static int aggr_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint32_t* d_key_idx, size_t m, const uint8_t* d_sigs,
                       const uint64_t* d_agg_off, size_t n, uint32_t flags, const uint8_t* seed32, uint8_t* d_status, hipStream_t s) {
  const uint32_t dflags = flags & (BN254_FLAG_G2_SUBGROUP_CHECK | BN254_FLAG_REJECT_IDENTITY);
  const size_t K = c->n_keys, G = (size_t)c->agg_rand_group_pairs > K ? (size_t)c->agg_rand_group_pairs : K;
  const size_t ng = m / G + 1, n_b = ng * (K + 1), n_e = m + n;
  const size_t n_tp_max = m < ng * K ? m : ng * K;                          // table pairs: one per non-empty (group, key) bucket
  const int kr = c->aggd_keyed_route;
  const int wx = kr == 1 || kr == 2 ? kr : m + n <= AGGD_KEYED_W1_MAX_SLOTS ? 1 : 2;     // the re-check: the exact call's slots
  const int wg = n_tp_max + ng <= AGGD_KEYED_W1_MAX_SLOTS ? 1 : 2;                       // the group checks: the same rule on their bound
  const size_t n_xslots = wx == 1 ? m + n : m / 2 + n, n_gslots = wg == 1 ? n_tp_max + ng : n_tp_max / 2 + ng;
  const size_t px = aggd_partials(n_xslots), pg = aggd_partials(n_gslots), n_part = px > pg ? px : pg, n_spart = aggr_partials(n_e);
  const size_t pbase = round256(m + 1), gbase = round256(pbase + n_part > n ? pbase + n_part : n), cbase = round256(gbase + n);
  const size_t tbase = round256(cbase + ng);
  int rc = ws_reserve(c, tbase + n_tp_max);
  if (rc) return rc;
  const size_t nbmax = (std::max(std::max(n, n_b), ng) + AGGD_SCAN_WG - 1) / AGGD_SCAN_WG;
  const size_t u64_words = 5 * n + nbmax + 2 * n_b + 3 * ng;
  const size_t u32_words = 2 * n + m + n_xslots + n_part + ng + 3 * n_e + (tbase + n_tp_max) + n_gslots + n_spart;
  const size_t bytes = 8 * u64_words + 4 * u32_words + 4 * AGGR_PART_WORDS * n_spart + ng + n;
  if (bytes > c->aggr_cap) {
    if ((rc = ctx_quiesce(c))) return rc;
    if (c->aggr_buf) { HIP_TRY(hipFree(c->aggr_buf)); c->aggr_buf = nullptr; c->aggr_cap = 0; }
    const size_t cap = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc((void**)&c->aggr_buf, cap));
    c->aggr_cap = cap;
  }
  if (!c->aggr_stats) HIP_TRY(hipMalloc((void**)&c->aggr_stats, 8 * sizeof(uint32_t)));
  uint64_t* mx = (uint64_t*)c->aggr_buf;
  uint64_t *incl = mx + n, *lo = incl + n, *hi = lo + n, *kincl = hi + n, *tot = kincl + n, *cnt = tot + nbmax, *tp = cnt + n_b, *glo = tp + n_b;
  uint64_t *ghi = glo + ng, *gkincl = ghi + ng;
  uint32_t* first_pk = (uint32_t*)(gkincl + ng);
  uint32_t *first_hash = first_pk + n, *pair_agg = first_hash + n, *xseg0 = pair_agg + m, *pseg = xseg0 + n_xslots, *nagg = pseg + n_part;
  uint32_t *ebkt = nagg + ng, *perm = ebkt + n_e, *eseg = perm + n_e, *bkey = eseg + n_e, *gseg0 = bkey + tbase + n_tp_max, *spseg = gseg0 + n_gslots;
  int32_t* part = (int32_t*)(spseg + n_spart);
  uint8_t* gst = (uint8_t*)(part + AGGR_PART_WORDS * n_spart);
  uint8_t* queued = gst + ng;
  const KeyTable kt = {c->key_lines, c->key_st, c->key_inf, (uint32_t)K};
  uint32_t seed_w[8];
  for (int j = 0; j < 8; ++j)
    seed_w[j] = ((uint32_t)seed32[4 * j] << 24) | ((uint32_t)seed32[4 * j + 1] << 16) | ((uint32_t)seed32[4 * j + 2] << 8) | seed32[4 * j + 3];
  const int mode = (flags & BN254_FLAG_RAND64) ? 1 : (flags & BN254_FLAG_RAND_GLV) ? 2 : 0;
  CallDone call_done(c, s);
  c->aggr_last = {ng, cbase, tbase, nagg, bkey, glo, ghi, gst};   // nothing below rewrites these once the group checks are through
  PROF_MARK(0);
  // 1-3: as the exact keyed call (bn254_aggdist.hip: aggd_device), with each pair's aggregate for the G1 side
  if ((rc = launch_decode_g1(c, s, d_sigs, n, dflags, PL_P2X, BY_P2_INF, 0))) return rc;
  if ((rc = aggd_scan<AggdMax>(s, d_agg_off, n, mx, tot))) return rc;
  k_aggd_prep<<<grid_for(n), BN_WAVE, 0, s>>>(n, (uint64_t)m, d_agg_off, mx, incl, lo, hi, first_pk, first_hash, c->ws, gbase);
  if ((rc = aggd_scan<AggdAdd>(s, incl, n, incl, tot))) return rc;
  k_aggd_keyed_count<<<grid_for(n), BN_WAVE, 0, s>>>(n, lo, hi, (uint64_t)wx, kincl);
  if ((rc = aggd_scan<AggdAdd>(s, kincl, n, kincl, tot))) return rc;
  k_aggd_keyed_keys<<<grid_for(m), BN_WAVE, 0, s>>>(m, d_key_idx, kt, c->key_xy, c->ws, 0);
  HIP_TRY(hipGetLastError());
  PROF_MARK(1);
  if ((rc = launch_hash_rounds(c, s, d_msgs, d_msg_off, m, PL_P1X, BY_P1_INF, nullptr))) return rc;
  PROF_MARK(2);
  HIP_TRY(hipMemsetAsync(pair_agg, 0xFF, 4 * m, s));
  const size_t n_slots = (m + n + 1) / 2;
  k_aggd_map<<<grid_for(n_slots), BN_WAVE, 0, s>>>(n_slots, n, incl, lo, hi, nullptr, pair_agg, first_pk, first_hash, c->ws);
  k_aggd_keyed_map<<<grid_for(n_xslots), BN_WAVE, 0, s>>>(n_xslots, n, kincl, xseg0);
  k_aggd_status<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws, gbase, first_pk, first_hash);
  // the G1 side: scaled entries counted by bucket, sorted, summed into the groups' table pairs and S_g
  HIP_TRY(hipMemsetAsync(nagg, 0, 4 * ng, s));
  HIP_TRY(hipMemsetAsync(cnt, 0, 8 * n_b, s));
  HIP_TRY(hipMemsetAsync(eseg, 0xFF, 4 * n_e, s));
  const AggrScale sc = {pair_agg, d_key_idx, c->key_inf, lo, nagg, ebkt, cnt, (uint64_t)G, (uint32_t)K};
  if ((rc = bn254_aggr_scale(m, n, c->ws, gbase, sc, seed_w, mode, s))) return rc;
  if ((rc = aggd_scan<AggdAdd>(s, cnt, n_b, tp, tot))) return rc;
  if ((rc = bn254_aggr_scatter(n_e, ebkt, tp, perm, eseg, n_b, (uint32_t)K, cnt, tp, s))) return rc;
  if ((rc = aggd_scan<AggdAdd>(s, tp, n_b, tp, tot))) return rc;
  if ((rc = bn254_aggr_glimits(ng, (uint32_t)K, tbase, cnt, tp, glo, ghi, c->ws, cbase, s))) return rc;
  const AggrSum sm = {perm, tp, bkey, m, gbase, cbase, tbase, (uint32_t)K};
  {
    size_t e = n_e, off = 0;
    const uint32_t* seg_in = eseg;
    const int32_t* part_in = nullptr;
    for (bool first = true;; first = false) {
      const size_t g = (e + AGGR_SUM_WG - 1) / AGGR_SUM_WG;
      const int last = g <= 1;
      if ((rc = bn254_aggr_sum(e, first, c->ws, sm, seg_in, part_in, spseg + off, part + AGGR_PART_WORDS * off, last, s))) return rc;
      if (last) break;
      seg_in = spseg + off;
      part_in = part + AGGR_PART_WORDS * off;
      e = 2 * g;
      off += 2 * g;
    }
  }
  PROF_MARK(3);                                        // ms[2] = hash .. sums, ms[3] = group checks, collect and re-check
  // one check per group: its table pairs and (S_g, -G2) through the slot kernel, the levels, the final exponentiation at index g
  k_aggd_keyed_count<<<grid_for(ng), BN_WAVE, 0, s>>>(ng, glo, ghi, (uint64_t)wg, gkincl);
  if ((rc = aggd_scan<AggdAdd>(s, gkincl, ng, gkincl, tot))) return rc;
  k_aggd_keyed_map<<<grid_for(n_gslots), BN_WAVE, 0, s>>>(n_gslots, ng, gkincl, gseg0);
  const AggdSlots gsl = {gseg0, gkincl, glo, ghi};
  if ((rc = aggd_levels(c, s, n_gslots, cbase, pbase, pseg, [&](size_t e, size_t pb, uint32_t* ps, int last) {
         return bn254_pair_aggd_keyed_queued(e, wg, c->ws, gsl, bkey, kt, cbase, pb, ps, last, nullptr, s);   // empty workgroups leave
       })))
    return rc;
  if ((rc = bn254_pair_aggd_move(ng, c->ws, cbase, s))) return rc;
  if ((rc = launch_final_exp_layout(c, s, ng, 0, gst, route_for(c, ng).fe))) return rc;
  // statuses; the aggregates of failed groups (of two or more) queued and checked exactly — with none queued, launches that leave at once
  HIP_TRY(hipMemsetAsync(c->ws.h_cnt, 0, sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(c->aggr_stats, 0, 8 * sizeof(uint32_t), s));
  if ((rc = bn254_aggr_collect(n, c->ws, gbase, lo, (uint64_t)G, nagg, gst, d_status, queued, ng, glo, ghi, c->aggr_stats, s))) return rc;
  const AggdSlots xsl = {xseg0, kincl, lo, hi};
  if ((rc = aggd_levels(c, s, n_xslots, gbase, pbase, pseg, [&](size_t e, size_t pb, uint32_t* ps, int last) {
         return bn254_pair_aggd_keyed_queued(e, wx, c->ws, xsl, d_key_idx, kt, gbase, pb, ps, last, queued, s);
       })))
    return rc;
  if ((rc = bn254_pair_aggd_move(n, c->ws, gbase, s))) return rc;
  if ((rc = bn254_pair_final_exp(n, c->ws, 0, d_status, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  PROF_MARK(4);
  if (c->profiling) { c->ev_valid = 1; c->ev_hash_first = 0; }
  HIP_TRY(hipGetLastError());
  c->aggr_last_ran = 1;                                // only a call that enqueued everything has something for the debug hooks to read
  return 0;
}

extern "C" {

int bn254_batch_aggregate_verify_distinct_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_pks, size_t m,
                                                 const uint8_t* d_agg_sigs, const uint64_t* d_agg_off, size_t n, uint32_t flags, uint8_t* d_status,
                                                 void* stream) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || !d_agg_off || (n && (!d_agg_sigs || !d_status)) || (m && (!d_msgs || !d_msg_off || !d_pks))) return BN254_E_BAD_ARGUMENT;
  if (m > 0xFFFFFFFFu || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_agg_sigs) || misaligned(d_pks) || ((uintptr_t)d_msg_off & 7u) || ((uintptr_t)d_agg_off & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  return aggd_device(c, d_msgs, d_msg_off, d_pks, false, nullptr, m, d_agg_sigs, d_agg_off, n, flags, d_status, stream ? (hipStream_t)stream : c->stream);
}

int bn254_batch_aggregate_verify_distinct(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pks, size_t m, const uint8_t* agg_sigs,
                                          const uint64_t* agg_off, size_t n, uint32_t flags, uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || !msg_off || !agg_off || (n && (!agg_sigs || !status)) || (m && !pks)) return BN254_E_BAD_ARGUMENT;
  if (m > 0xFFFFFFFFu || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (agg_off[0] != 0 || agg_off[n] != m || !offsets_ok(agg_off, n) || !offsets_ok(msg_off, m)) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, msg_off, m)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)msg_off[m]), *d_msg_off = st.in(1, msg_off, (m + 1) * sizeof(uint64_t));
  const uint8_t *d_pks = st.in(2, pks, m * 128), *d_agg_sigs = st.in(3, agg_sigs, n * 64), *d_agg_off = st.in(4, agg_off, (n + 1) * sizeof(uint64_t));
  uint8_t* d_status = st.out(5, n, status);
  if (st.ok())
    st.rc = bn254_batch_aggregate_verify_distinct_device(c, d_msgs, (const uint64_t*)d_msg_off, d_pks, m, d_agg_sigs, (const uint64_t*)d_agg_off, n, flags,
                                                         d_status, nullptr);
  return st.finish();
}

// ---- registered keys: pk_j = registered[key_idx[j]] (include/bn254_hip.h) -------------------------------------------------------------------
int bn254_batch_aggregate_verify_distinct_keyed_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint32_t* d_key_idx, size_t m,
                                                       const uint8_t* d_agg_sigs, const uint64_t* d_agg_off, size_t n, uint32_t flags, uint8_t* d_status,
                                                       void* stream) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || !d_agg_off || (n && (!d_agg_sigs || !d_status)) || (m && (!d_msgs || !d_msg_off || !d_key_idx))) return BN254_E_BAD_ARGUMENT;
  if (m > 0xFFFFFFFFu || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_agg_sigs) || misaligned(d_key_idx) || ((uintptr_t)d_msg_off & 7u) || ((uintptr_t)d_agg_off & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  return aggd_device(c, d_msgs, d_msg_off, nullptr, true, d_key_idx, m, d_agg_sigs, d_agg_off, n, flags, d_status, stream ? (hipStream_t)stream : c->stream);
}

int bn254_batch_aggregate_verify_distinct_keyed(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* key_idx, size_t m,
                                                const uint8_t* agg_sigs, const uint64_t* agg_off, size_t n, uint32_t flags, uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || !msg_off || !agg_off || (n && (!agg_sigs || !status)) || (m && !key_idx)) return BN254_E_BAD_ARGUMENT;
  if (m > 0xFFFFFFFFu || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (agg_off[0] != 0 || agg_off[n] != m || !offsets_ok(agg_off, n) || !offsets_ok(msg_off, m)) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, msg_off, m)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)msg_off[m]), *d_msg_off = st.in(1, msg_off, (m + 1) * sizeof(uint64_t));
  const uint8_t *d_key_idx = st.in(2, key_idx, m * sizeof(uint32_t)), *d_agg_sigs = st.in(3, agg_sigs, n * 64);
  const uint8_t* d_agg_off = st.in(4, agg_off, (n + 1) * sizeof(uint64_t));
  uint8_t* d_status = st.out(5, n, status);
  if (st.ok())
    st.rc = bn254_batch_aggregate_verify_distinct_keyed_device(c, d_msgs, (const uint64_t*)d_msg_off, (const uint32_t*)d_key_idx, m, d_agg_sigs,
                                                               (const uint64_t*)d_agg_off, n, flags, d_status, nullptr);
  return st.finish();
}

// ---- registered keys, randomised ----------------------------------------------------------------------------------------------------------
int bn254_batch_aggregate_verify_distinct_keyed_randomized_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint32_t* d_key_idx,
                                                                  size_t m, const uint8_t* d_agg_sigs, const uint64_t* d_agg_off, size_t n, uint32_t flags,
                                                                  const uint8_t* seed32, uint8_t* d_status, void* stream) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || !seed32 || !d_agg_off || (n && (!d_agg_sigs || !d_status)) || (m && (!d_msgs || !d_msg_off || !d_key_idx))) return BN254_E_BAD_ARGUMENT;
  if (m > 0xFFFFFFFFu || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  c->aggr_last_ran = 0;
  if (n == 0) return 0;
  if (misaligned(d_agg_sigs) || misaligned(d_key_idx) || ((uintptr_t)d_msg_off & 7u) || ((uintptr_t)d_agg_off & 7u)) return BN254_E_MISALIGNED;
  // no keys, pair lanes off, too few messages (or none): the exact keyed call, same bytes; entries are numbered in 32 bits
  if (c->n_keys == 0 || !c->key_lines || !c->pair_lanes || m == 0 || m < (size_t)c->agg_rand_min_pairs || m + n > 0xFFFFFFFFu)
    return bn254_batch_aggregate_verify_distinct_keyed_device(c, d_msgs, d_msg_off, d_key_idx, m, d_agg_sigs, d_agg_off, n, flags, d_status, stream);
  HIP_TRY(hipSetDevice(c->device));
  return aggr_device(c, d_msgs, d_msg_off, d_key_idx, m, d_agg_sigs, d_agg_off, n, flags, seed32, d_status, stream ? (hipStream_t)stream : c->stream);
}

int bn254_batch_aggregate_verify_distinct_keyed_randomized(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint32_t* key_idx, size_t m,
                                                           const uint8_t* agg_sigs, const uint64_t* agg_off, size_t n, uint32_t flags, const uint8_t* seed32,
                                                           uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || !seed32 || !msg_off || !agg_off || (n && (!agg_sigs || !status)) || (m && !key_idx)) return BN254_E_BAD_ARGUMENT;
  if (m > 0xFFFFFFFFu || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (agg_off[0] != 0 || agg_off[n] != m || !offsets_ok(agg_off, n) || !offsets_ok(msg_off, m)) return BN254_E_BAD_ARGUMENT;
  c->aggr_last_ran = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, msg_off, m)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)msg_off[m]), *d_msg_off = st.in(1, msg_off, (m + 1) * sizeof(uint64_t));
  const uint8_t *d_key_idx = st.in(2, key_idx, m * sizeof(uint32_t)), *d_agg_sigs = st.in(3, agg_sigs, n * 64);
  const uint8_t* d_agg_off = st.in(4, agg_off, (n + 1) * sizeof(uint64_t));
  uint8_t* d_status = st.out(5, n, status);
  if (st.ok())
    st.rc = bn254_batch_aggregate_verify_distinct_keyed_randomized_device(c, d_msgs, (const uint64_t*)d_msg_off, (const uint32_t*)d_key_idx, m, d_agg_sigs,
                                                                          (const uint64_t*)d_agg_off, n, flags, seed32, d_status, nullptr);
  return st.finish();
}

}  // extern "C"
