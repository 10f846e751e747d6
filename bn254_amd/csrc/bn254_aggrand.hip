// Translation unit of libbn254hip.so: the kernels of the RANDOMISED batch verification of keyed aggregates over distinct messages
// (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed_randomized[_device]; host side: bn254_aggdist.hip, aggr_device).
// Compiled with the defines of bn254_pair.hip, as bn254_aggkeyed.hip is, for the re-check's slot kernel.
//
// A group g of whole aggregates passes iff
//     prod_key e(sum_{i in g} r_i sum_{j in i, key_j = key} H(m_j), pk_key) * e(sum_{i in g} r_i sigma_i, -G2) == 1
// over its aggregates at the check.  Pipeline, behind the exact call's decode, prep, key statuses, hash and status fold:
//   k_aggr_groups   aggregates at the check per group;
//   k_aggr_scale    A_j = r_i H(m_j) and r_i sigma_i (r = 1 in a group of one), Jacobian, into the P2 / HASH planes; counts per (group, key)
//                   bucket — H(m_j) and sigma_i stay in the P1 planes for the re-check;
//   k_aggr_scatter  counting sort of the entries by bucket (positions from the scanned counts);
//   k_aggr_sum<L0>  segmented sums of the sorted entries: runs of one bucket reduced by a tree in LDS per workgroup, the first and last run
//                   of a workgroup left as partials for the next level (the scheme of aggd_reduce on G1); a whole bucket lands as an affine
//                   TABLE PAIR (P1 planes at tbase + its rank among the non-empty key buckets, key beside it) or, for the signature bucket,
//                   as S_g at cbase + g;
//   then the exact call's slot loop, levels and final exponentiation over the groups' table pairs (bn254_aggkeyed.hip), and
//   k_aggr_collect  statuses: group passed -> 0, group of one -> its verdict, else the aggregate is queued for
//   k_aggd_keyed_pair_q  the exact slot kernel on the original pairs, for queued aggregates only (a workgroup with nothing queued leaves
//                   before its Miller loop), the levels and the final exponentiation of the queue.
// The group checks run k_aggd_keyed_pair_q too, with no queue: their slot grid is a host-side bound, and its unused workgroups leave at once.
#include <hip/hip_runtime.h>

#define BN_SPLIT_FP2 1
#if defined(BN_PAIR_FP6_LAZY) && !defined(BN_FP6_LAZY)
#define BN_FP6_LAZY 1
#endif
#ifndef BN_PAIR_NO_SQR_DPP_ASM
#define BN_PAIR_SQR_DPP_ASM 1
#endif
#ifndef BN_PAIR_CALL_FP12_HOT
#define BN_INLINE_FP12_HOT 1
#endif
#ifndef BN_PAIR_CALL_MUL_LINE
#define BN_INLINE_MUL_LINE 1
#endif
#ifndef BN_PAIR_CALL_FE_HOT
#define BN_INLINE_FE_HOT 1
#endif
#ifndef BN_PRIO_SHIFT
#define BN_PRIO_SHIFT 1
#endif
#define BN_SET_STEP_PRIORITY(step)                                                        \
  do {                                                                                    \
    if (((step) & ((1 << BN_PRIO_SHIFT) - 1)) == 0) {                                     \
      int q_ = ((step) >> BN_PRIO_SHIFT) & 3;                                             \
      if (q_ == 0) __builtin_amdgcn_s_setprio(3);                                         \
      else if (q_ == 1) __builtin_amdgcn_s_setprio(2);                                    \
      else if (q_ == 2) __builtin_amdgcn_s_setprio(1);                                    \
      else __builtin_amdgcn_s_setprio(0);                                                 \
    }                                                                                     \
  } while (0)
#define bn254 bn254_aggr   // own namespace, as in bn254_fe.hip
#include "bn254_pairing.h"
#include "bn254_hash.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_aggrand.h"

#ifndef BN_PAIR_WG
#define BN_PAIR_WG 256
#endif
#define KERNEL_PAIR __global__ __launch_bounds__(BN_PAIR_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
#define KERNEL_SUM __global__ __launch_bounds__(AGGR_SUM_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))

#include "bn254_aggd_slot.h"

struct G1JacSlot { G1Jac v; int32_t pad; };   // as the randomised verify's LDS slots
struct AggrSeed { uint32_t w[8]; };

// ---- grouping and scaling (one lane per aggregate / entry) -------------------------------------------------------------------------------
KERNEL_SMALL void k_aggr_groups(size_t n, Ws ws, size_t gbase, AggrScale a) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n || ws_byte(ws, BY_ST_DECODE, gbase + i) != ST_OK) return;
  atomicAdd(&a.nagg[aggr_group(a.lo[i], a.G)], 1u);
}
// Entry v < m: message v of aggregate pair_agg[v] (H in the P1 planes at v); v >= m: the signature of aggregate v - m (P1 at gbase + v - m).
// An entry takes part iff its aggregate is at the check and its key is not the identity; its scaled point goes to the P2X / P2Y / HASHX
// planes at the same index (x, y, z), its bucket to ebkt[v].
__device__ __forceinline__ size_t aggr_entry_index(uint32_t v, size_t m, size_t gbase) { return v < m ? (size_t)v : gbase + (v - m); }
KERNEL_SMALL void k_aggr_scale(size_t m, size_t n, Ws ws, size_t gbase, AggrScale a, AggrSeed seed, int mode) {
  const size_t v = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  __shared__ G1JacSlot lds[BN_WAVE];                   // the ladder's accumulator in LDS, as in k_krand_scale
  if (v >= m + n) return;                               // no barrier below
  const bool is_sig = v >= m;
  const uint32_t agg = is_sig ? (uint32_t)(v - m) : a.pair_agg[v];
  const uint32_t key = is_sig ? a.n_keys : a.key_idx[v];
  bool live = agg != AGGR_NONE && ws_byte(ws, BY_ST_DECODE, gbase + agg) == ST_OK;
  if (live && !is_sig) live = a.key_inf[key] == 0;     // at the check, every key of the aggregate is registered and in range
  a.ebkt[v] = AGGR_NONE;
  if (!live) return;
  const uint64_t g = aggr_group(a.lo[agg], a.G);
  const size_t idx = aggr_entry_index((uint32_t)v, m, gbase);
  G1Affine p;
  ws_load_g1(ws, PL_P1X, BY_P1_INF, idx, p);
  G1Jac& acc = lds[threadIdx.x].v;
  aggr_scale(acc, p, seed.w, agg, mode, a.nagg[g] == 1);
  const G1Jac r = acc;
  ws_store_fp(ws, PL_P2X, idx, r.x);
  ws_store_fp(ws, PL_P2Y, idx, r.y);
  ws_store_fp(ws, PL_HASHX, idx, r.z);
  const uint64_t b = aggr_bucket(g, key, a.n_keys);
  a.ebkt[v] = (uint32_t)b;
  atomicAdd((unsigned long long*)&a.cnt[b], 1ull);
}
// start = the inclusive scan of the counts: every entry takes the last free position of its bucket (start ends as the exclusive scan)
KERNEL_SMALL void k_aggr_scatter(size_t n_entries, const uint32_t* ebkt, uint64_t* start, uint32_t* perm, uint32_t* eseg) {
  const size_t v = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (v >= n_entries) return;
  const uint32_t b = ebkt[v];
  if (b == AGGR_NONE) return;
  const uint64_t pos = atomicAdd((unsigned long long*)&start[b], ~0ull) - 1;
  perm[pos] = (uint32_t)v;
  eseg[pos] = b;
}
// the table pairs: 1 per non-empty KEY bucket (scanned next: rank + 1 of the bucket among them)
KERNEL_SMALL void k_aggr_nonempty(size_t n_b, uint32_t n_keys, const uint64_t* cnt, uint64_t* tp) {
  const size_t b = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (b >= n_b) return;
  tp[b] = cnt[b] != 0 && b % ((size_t)n_keys + 1) != n_keys;
}
// group g's table pairs [glo, ghi) (absolute workspace indices from tbase), its status byte for the final exponentiation, and S_g = the
// identity where no signature takes part (a group with no aggregate at the check: its one slot multiplies nothing)
KERNEL_SMALL void k_aggr_glimits(size_t n_groups, uint32_t n_keys, size_t tbase, const uint64_t* cnt, const uint64_t* tp, uint64_t* glo, uint64_t* ghi,
                                 Ws ws, size_t cbase) {
  const size_t g = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (g >= n_groups) return;
  const size_t b0 = g * ((size_t)n_keys + 1);
  glo[g] = tbase + (g ? tp[b0 - 1] : 0);
  ghi[g] = tbase + tp[b0 + n_keys];
  ws_byte(ws, BY_ST_DECODE, cbase + g) = ST_OK;
  if (cnt[b0 + n_keys] == 0) {
    G1Affine id;
    id.x = fp_zero(); id.y = fp_zero(); id.inf = true;
    ws_store_g1(ws, PL_P1X, BY_P1_INF, cbase + g, id);
  }
}

// ---- segmented sums of the sorted entries ------------------------------------------------------------------------------------------------
// One element per lane, AGGR_SUM_WG per workgroup, its id = its bucket (AGGR_NONE: nobody).  Round d of the tree: the element at run
// position r with r % 2d == 0 adds the one d further on if that is still in the run (an operand is never rewritten in the round that reads
// it).  A run that neither starts the workgroup nor reaches its end is a whole bucket; the first and the last run are the workgroup's two
// partials (Jacobian records at 2 block and 2 block + 1 of the level's output, ids beside them; the second is the identity when one run
// covers the workgroup).  last = 1: one workgroup, every run whole.  A workgroup of nobody leaves at once (its partials say so).
__device__ __forceinline__ void aggr_part_store(int32_t* part, size_t e, const G1Jac& p) {
  int32_t* w = part + e * AGGR_PART_WORDS;
  for (int k = 0; k < BN_LIMBS; ++k) { w[k] = p.x.v[k]; w[BN_LIMBS + k] = p.y.v[k]; w[2 * BN_LIMBS + k] = p.z.v[k]; }
}
__device__ __forceinline__ void aggr_part_load(const int32_t* part, size_t e, G1Jac& p) {
  const int32_t* w = part + e * AGGR_PART_WORDS;
  for (int k = 0; k < BN_LIMBS; ++k) { p.x.v[k] = w[k]; p.y.v[k] = w[BN_LIMBS + k]; p.z.v[k] = w[2 * BN_LIMBS + k]; }
}
template <bool L0>
KERNEL_SUM void k_aggr_sum(size_t n_elems, Ws ws, AggrSum a, const uint32_t* seg_in, const int32_t* part_in, uint32_t* pseg_out, int32_t* part_out,
                           int last) {
  const unsigned t = threadIdx.x;
  const size_t e = (size_t)blockIdx.x * AGGR_SUM_WG + t;
  const uint32_t seg = e < n_elems ? seg_in[e] : AGGR_NONE;
  __shared__ G1JacSlot lds[AGGR_SUM_WG];
  __shared__ uint32_t lds_seg[AGGR_SUM_WG];
  if (!__syncthreads_or(seg != AGGR_NONE)) {
    if (!last && t < 2) pseg_out[2 * (size_t)blockIdx.x + t] = AGGR_NONE;
    return;
  }
  G1Jac& p = lds[t].v;
  if (seg == AGGR_NONE) {
    jac_set_identity(p);
  } else if constexpr (L0) {
    const size_t idx = aggr_entry_index(a.perm[e], a.m, a.gbase);
    p.x = ws_load_fp(ws, PL_P2X, idx); p.y = ws_load_fp(ws, PL_P2Y, idx); p.z = ws_load_fp(ws, PL_HASHX, idx);
  } else {
    aggr_part_load(part_in, e, p);
  }
  lds_seg[t] = seg;
  __syncthreads();
  unsigned head = 0, hi = t;                           // the first element of this run (the ids of a run are contiguous)
  while (head < hi) {
    const unsigned mid = (head + hi) >> 1;
    if (lds_seg[mid] == seg) hi = mid; else head = mid + 1;
  }
  const unsigned r = t - head;
  for (unsigned d = 1; d < AGGR_SUM_WG; d <<= 1) {
    if (seg != AGGR_NONE && (r & (2 * d - 1)) == 0 && t + d < AGGR_SUM_WG && lds_seg[t + d] == seg) jac_add(lds[t].v, lds[t].v, lds[t + d].v);
    __syncthreads();
  }
  if (t != 0 && lds_seg[t - 1] == seg) return;          // not the head of its run
  const bool first = t == 0, reaches_end = lds_seg[AGGR_SUM_WG - 1] == seg;
  if (last || (!first && !reaches_end)) {
    if (seg == AGGR_NONE) return;
    const uint64_t g = seg / ((uint64_t)a.n_keys + 1);
    const uint32_t key = (uint32_t)(seg - g * ((uint64_t)a.n_keys + 1));
    G1Affine s;
    jac_to_affine(s, lds[t].v);
    if (key == a.n_keys) {
      ws_store_g1(ws, PL_P1X, BY_P1_INF, a.cbase + g, s);
    } else {
      const size_t at = a.tbase + a.tp[seg] - 1;
      ws_store_g1(ws, PL_P1X, BY_P1_INF, at, s);
      a.bkey[at] = key;
    }
    return;
  }
  const size_t p0 = 2 * (size_t)blockIdx.x;
  G1Jac v = lds[t].v;
  if (first) {
    aggr_part_store(part_out, p0, v);
    pseg_out[p0] = seg;
    if (!reaches_end) return;
    jac_set_identity(v);                               // one run covers the workgroup: the second partial is the identity
  }
  aggr_part_store(part_out, p0 + 1, v);
  pseg_out[p0 + 1] = seg;
}

// ---- statuses and the re-check queue -----------------------------------------------------------------------------------------------------
KERNEL_SMALL void k_aggr_collect(size_t n, Ws ws, size_t gbase, const uint64_t* lo, uint64_t G, const uint32_t* nagg, const uint8_t* gst, uint8_t* status,
                                 uint8_t* queued) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = ws_byte(ws, BY_ST_DECODE, gbase + i);
  queued[i] = 0;
  if (st != ST_OK) { status[i] = st; return; }
  const uint64_t g = aggr_group(lo[i], G);
  if (nagg[g] == 1 || gst[g] == ST_OK) { status[i] = gst[g]; return; }   // a group of one is the exact check itself
  queued[i] = 1;
  ws.h_list[atomicAdd(&ws.h_cnt[0], 1u)] = (uint32_t)i;
}
// bn254_debug_agg_rand_last: {groups at the check, their table pairs, failed groups, aggregates re-checked, groups of one}
KERNEL_SMALL void k_aggr_stats(size_t n_groups, const uint32_t* nagg, const uint64_t* glo, const uint64_t* ghi, const uint8_t* gst, const uint32_t* h_cnt,
                               uint32_t* stats) {
  const size_t g = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (g == 0) stats[3] = h_cnt[0];
  if (g >= n_groups || nagg[g] == 0) return;
  atomicAdd(&stats[0], 1u);
  atomicAdd(&stats[1], (uint32_t)(ghi[g] - glo[g] + 1));
  if (nagg[g] > 1 && gst[g] != ST_OK) atomicAdd(&stats[2], 1u);
  if (nagg[g] == 1) atomicAdd(&stats[4], 1u);
}

// ---- the slot kernel of bn254_aggkeyed.hip for workgroups with work only ----------------------------------------------------------------
// queued != null: the exact re-check, for the aggregates marked there only.  queued = null: the group checks, whose slot grid is sized from
// a host-known bound (slots past the device-side count are nobody's).  A workgroup with no live slot leaves before its Miller loop.
template <int W>
KERNEL_PAIR void k_aggd_keyed_pair_q(size_t n_slots, Ws ws, AggdSlots sl, const uint32_t* key_idx, KeyTable kt, size_t gbase, size_t pbase, uint32_t* pseg,
                                     int last, const uint8_t* queued) {
  const size_t e = ((size_t)blockIdx.x * BN_PAIR_WG + threadIdx.x) >> 1;
  uint32_t seg = e < n_slots ? sl.slot_agg[e] : AGGD_SEG_NONE;
  if (seg != AGGD_SEG_NONE && queued && !queued[seg]) seg = AGGD_SEG_NONE;
  if (!__syncthreads_or(seg != AGGD_SEG_NONE)) {         // nothing queued here: no Miller loop, the partials belong to nobody
    if (!last && threadIdx.x < 2) pseg[2 * (size_t)blockIdx.x + threadIdx.x] = AGGD_SEG_NONE;
    return;
  }
  uint64_t lo = 0, k = 0, t0 = 0;
  if (seg != AGGD_SEG_NONE) {
    lo = sl.lo[seg];
    k = sl.hi[seg] - lo;
    t0 = W * (e - (sl.incl[seg] - (k + W) / W));
  }
  const AggdTablePair a = aggd_table_pair(ws, key_idx, kt, seg, lo, k, t0, gbase);
  __shared__ Fp12PairSlot lds_f[BN_PAIR_WG];
  __shared__ uint32_t lds_seg[AGGD_WG_ELEMS];
  if constexpr (W == 2) {
    const AggdTablePair b = aggd_table_pair(ws, key_idx, kt, seg, lo, k, t0 + 1, gbase);
    miller_loop_tables<2, true>(lds_f[threadIdx.x].v, a.p, a.skip, a.tab, b.p, b.skip, b.tab);
  } else {
    miller_loop_tables<1, true>(lds_f[threadIdx.x].v, a.p, a.skip, a.tab, a.p, true, a.tab);
  }
  aggd_reduce(lds_f, lds_seg, seg, ws, gbase, pbase, pseg, last);
}

// ---- launchers (bn254_ws.h) --------------------------------------------------------------------------------------------------------------
int bn254_aggr_scale(size_t m, size_t n, Ws ws, size_t gbase, AggrScale a, const uint32_t* seed_be, int mode, hipStream_t s) {
  AggrSeed seed;
  for (int j = 0; j < 8; ++j) seed.w[j] = seed_be[j];
  k_aggr_groups<<<(unsigned)((n + BN_WAVE - 1) / BN_WAVE), BN_WAVE, 0, s>>>(n, ws, gbase, a);
  k_aggr_scale<<<(unsigned)((m + n + BN_WAVE - 1) / BN_WAVE), BN_WAVE, 0, s>>>(m, n, ws, gbase, a, seed, mode);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_aggr_scatter(size_t n_entries, const uint32_t* ebkt, uint64_t* start, uint32_t* perm, uint32_t* eseg, size_t n_b, uint32_t n_keys,
                       const uint64_t* cnt, uint64_t* tp, hipStream_t s) {
  k_aggr_scatter<<<(unsigned)((n_entries + BN_WAVE - 1) / BN_WAVE), BN_WAVE, 0, s>>>(n_entries, ebkt, start, perm, eseg);
  k_aggr_nonempty<<<(unsigned)((n_b + BN_WAVE - 1) / BN_WAVE), BN_WAVE, 0, s>>>(n_b, n_keys, cnt, tp);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_aggr_glimits(size_t n_groups, uint32_t n_keys, size_t tbase, const uint64_t* cnt, const uint64_t* tp, uint64_t* glo, uint64_t* ghi, Ws ws,
                       size_t cbase, hipStream_t s) {
  k_aggr_glimits<<<(unsigned)((n_groups + BN_WAVE - 1) / BN_WAVE), BN_WAVE, 0, s>>>(n_groups, n_keys, tbase, cnt, tp, glo, ghi, ws, cbase);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_aggr_sum(size_t n_elems, int level0, Ws ws, AggrSum a, const uint32_t* seg_in, const int32_t* part_in, uint32_t* pseg_out, int32_t* part_out,
                   int last, hipStream_t s) {
  const unsigned g = (unsigned)((n_elems + AGGR_SUM_WG - 1) / AGGR_SUM_WG);
  if (level0) k_aggr_sum<true><<<g, AGGR_SUM_WG, 0, s>>>(n_elems, ws, a, seg_in, part_in, pseg_out, part_out, last);
  else k_aggr_sum<false><<<g, AGGR_SUM_WG, 0, s>>>(n_elems, ws, a, seg_in, part_in, pseg_out, part_out, last);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_aggr_collect(size_t n, Ws ws, size_t gbase, const uint64_t* lo, uint64_t G, const uint32_t* nagg, const uint8_t* gst, uint8_t* status,
                       uint8_t* queued, size_t n_groups, const uint64_t* glo, const uint64_t* ghi, uint32_t* stats, hipStream_t s) {
  k_aggr_collect<<<(unsigned)((n + BN_WAVE - 1) / BN_WAVE), BN_WAVE, 0, s>>>(n, ws, gbase, lo, G, nagg, gst, status, queued);
  k_aggr_stats<<<(unsigned)((n_groups + BN_WAVE - 1) / BN_WAVE), BN_WAVE, 0, s>>>(n_groups, nagg, glo, ghi, gst, ws.h_cnt, stats);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_pair_aggd_keyed_queued(size_t n_slots, int width, Ws ws, AggdSlots sl, const uint32_t* key_idx, KeyTable kt, size_t gbase, size_t pbase,
                                 uint32_t* pseg, int last, const uint8_t* queued, hipStream_t s) {
  const unsigned g = (unsigned)((n_slots + AGGD_WG_ELEMS - 1) / AGGD_WG_ELEMS);
  if (width == 1) k_aggd_keyed_pair_q<1><<<g, BN_PAIR_WG, 0, s>>>(n_slots, ws, sl, key_idx, kt, gbase, pbase, pseg, last, queued);
  else k_aggd_keyed_pair_q<2><<<g, BN_PAIR_WG, 0, s>>>(n_slots, ws, sl, key_idx, kt, gbase, pbase, pseg, last, queued);
  HIP_TRY(hipGetLastError());
  return 0;
}
