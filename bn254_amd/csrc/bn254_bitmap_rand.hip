// Translation unit of libbn254hip.so: the RANDOMISED batch verification of same-message aggregates given as signer bitmaps over the
// registered keys (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap_randomized[_device]) — its kernels and its host side.
// Compiled with the Fq2 layout of bn254_pair.hip, as bn254_bitmap_pair.hip is, for the re-check's aggregate keys on lane pairs.
//
// Every aggregate key is a sum over the registered set, so the combined check of a group g of tuples regroups by key:
//     prod_j e(T_{g,j}, pk_j) * e(S_g, -G2) == 1,   T_{g,j} = sum_{i in g, bit j of i} r_i H(m_i),   S_g = sum_{i in g} r_i sigma_i
// — n_keys + 1 table-driven Miller pairs and one final exponentiation per group.  Pipeline, behind sigma's decode and the hash:
//   k_bmr_status     rules 1-3 folded into the tuple's status byte; tuples at the check counted per group;
//   k_bmr_scale      r_i H(m_i) and r_i sigma_i (r = 1 in a group of one; the ladders of bn254_aggrand.h), Jacobian, behind the tuples; one
//                    sort element per non-zero bitmap byte, in byte bucket (g, w, v), and one in S_g's bucket (bn254_bitmap_rand.h);
//   the counting sort and the segmented sums of the distinct-message call (bn254_aggrand.hip), k_bmr_perm_points in between: a sort
//                    element names its point;
//   k_bmr_keymask    per (g, w) the keys with a contributor; scanned: the places of the groups' table pairs; k_bmr_glimits;
//   k_bmr_fold       per (g, w) the 255 bucket sums folded into its key sums, each written as an affine table pair;
//   then the slot kernel, the levels and the final exponentiation over the groups (as the distinct-message call's group checks), the
//   collect of that call, and for the tuples of failed groups
//   k_bmr_sum_pair_q the exact aggregate key (bn254_bitmap.h's walk) of the queued tuples only, and a verify of the queue.
#include <hip/hip_runtime.h>

#define BN_SPLIT_FP2 1
#ifndef BN_PAIR_NO_SQR_DPP_ASM
#define BN_PAIR_SQR_DPP_ASM 1
#endif
#define bn254 bn254_bmr   // own namespace, as in bn254_fe.hip
#include "bn254_pairing.h"
#include "bn254_hash.h"
#include "bn254_bitmap.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_aggrand.h"
#include "bn254_bitmap_rand.h"
#include "bn254_host.h"
#include "bn254_aggd_plan.h"

#ifndef BN_PAIR_WG
#define BN_PAIR_WG 256
#endif
#define KERNEL_PAIR __global__ __launch_bounds__(BN_PAIR_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
#define BMR_FOLD_WG 256
#define KERNEL_FOLD __global__ __launch_bounds__(BMR_FOLD_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))

struct BmrSeed { uint32_t w[8]; };
struct BmrScale { const uint32_t* nagg; uint32_t* ebkt; uint64_t* cnt; uint64_t G, index_base; size_t ebase; uint32_t n_keys, nwin; };
struct BmrFold { const uint64_t* cnt; const uint64_t* tp; const uint64_t* tincl; const uint32_t* mask; uint32_t* bkey; size_t bpbase, tbase; uint32_t nW, n_keys; };

// ---- statuses and scaling (one lane per tuple / point) ------------------------------------------------------------------------------------
// rules 1-3 in the exact call's order: sigma's decode status, the lowest bad bit, the hash status.  lo[i] = i: the collect of the
// distinct-message call groups an aggregate by its first pair.
KERNEL_SMALL void k_bmr_status(size_t n, const uint32_t* bits, size_t bm_words, BmKeys K, Ws ws, uint64_t G, uint32_t* nagg, uint64_t* lo) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  uint8_t st = ws_byte(ws, BY_ST_DECODE, i);
  if (st == ST_OK) st = bm_rule2_status(bits + i * bm_words, bm_words, K);
  if (st == ST_OK) st = ws_byte(ws, BY_ST_HASH, i);
  ws_byte(ws, BY_ST_DECODE, i) = st;
  lo[i] = i;
  if (st == ST_OK) atomicAdd(&nagg[i / G], 1u);
}
// Point v < n: H(m_v) (P2 planes at v); v >= n: sigma of tuple v - n (P1 planes).  The scaled point goes to the P2X / P2Y / HASHX planes at
// ebase + v (x, y, z).  Sort element w n + i = byte w of tuple i (w < nwin), nwin n + i = its signature; ebkt = its bucket.
KERNEL_SMALL void k_bmr_scale(size_t n, const uint32_t* bits, size_t bm_words, Ws ws, BmrScale a, BmrSeed seed, int mode) {
  const size_t v = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  __shared__ BmrSlot lds[BN_WAVE];                     // the ladder's accumulator in LDS, as in k_aggr_scale
  if (v >= 2 * n) return;                              // no barrier below
  const bool is_sig = v >= n;
  const size_t i = is_sig ? v - n : v;
  if (ws_byte(ws, BY_ST_DECODE, i) != ST_OK) return;
  const uint64_t g = i / a.G;
  G1Affine p;
  ws_load_g1(ws, is_sig ? PL_P1X : PL_P2X, is_sig ? BY_P1_INF : BY_P2_INF, i, p);
  G1Jac& acc = lds[threadIdx.x].v;
  aggr_scale(acc, p, seed.w, a.index_base + i, mode, a.nagg[g] == 1);
  const G1Jac r = acc;
  ws_store_fp(ws, PL_P2X, a.ebase + v, r.x);
  ws_store_fp(ws, PL_P2Y, a.ebase + v, r.y);
  ws_store_fp(ws, PL_HASHX, a.ebase + v, r.z);
  if (is_sig) {
    const uint64_t b = bmr_sig_bucket(g, a.n_keys);
    a.ebkt[(size_t)a.nwin * n + i] = (uint32_t)b;
    atomicAdd((unsigned long long*)&a.cnt[b], 1ull);
    return;
  }
  const uint32_t* row = bits + i * bm_words;
  for (uint32_t w = 0; w < a.nwin; ++w) {
    const uint32_t byte = bmr_byte(row, bm_words, w);
    if (byte == 0) continue;
    const uint64_t b = bmr_bucket(g, w, byte, a.n_keys);
    a.ebkt[(size_t)w * n + i] = (uint32_t)b;
    atomicAdd((unsigned long long*)&a.cnt[b], 1ull);
  }
}
// after the scatter: a sorted element names its sort element; the sums read a point, so it becomes the point's number (eseg tells a
// position in use from one past the end)
KERNEL_SMALL void k_bmr_perm_points(size_t n_e, size_t n, uint32_t nwin, const uint32_t* eseg, uint32_t* perm) {
  const size_t e = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (e >= n_e || eseg[e] == AGGR_NONE) return;
  const size_t el = perm[e], w = el / n, i = el - w * n;
  perm[e] = (uint32_t)(w == nwin ? n + i : i);
}

// ---- the table pairs ----------------------------------------------------------------------------------------------------------------------
// (g, w): the keys of the window with a contributor = the union of the byte values of its non-empty buckets, less the keys that carry no
// pair (bmr_window_keys); their number, scanned next
KERNEL_SMALL void k_bmr_keymask(size_t n_gw, uint32_t nW, uint32_t n_keys, const uint8_t* key_st, const uint8_t* key_inf, const uint64_t* cnt,
                                uint32_t* mask, uint64_t* tcnt) {
  const size_t gw = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (gw >= n_gw) return;
  const uint64_t g = gw / nW;
  const uint32_t w = (uint32_t)(gw - g * nW);
  const uint64_t* c = cnt + bmr_bucket(g, w, 1, n_keys);
  uint32_t m = 0;
  for (uint32_t v = 1; v < 256; ++v) if (c[v - 1] != 0) m |= v;
  m &= bmr_window_keys(w, n_keys, key_st, key_inf);
  mask[gw] = m;
  tcnt[gw] = (uint64_t)__builtin_popcount(m);
}
// group g's table pairs [glo, ghi) (absolute workspace indices from tbase), its status byte for the final exponentiation, and S_g = the
// identity where no signature takes part (k_aggr_glimits with the pairs counted per window)
KERNEL_SMALL void k_bmr_glimits(size_t n_groups, uint32_t nW, uint32_t n_keys, size_t tbase, const uint64_t* cnt, const uint64_t* tincl, uint64_t* glo,
                                uint64_t* ghi, Ws ws, size_t cbase) {
  const size_t g = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (g >= n_groups) return;
  glo[g] = tbase + (g ? tincl[g * nW - 1] : 0);
  ghi[g] = tbase + tincl[(g + 1) * nW - 1];
  ws_byte(ws, BY_ST_DECODE, cbase + g) = ST_OK;
  if (cnt[bmr_sig_bucket(g, n_keys)] == 0) {
    G1Affine id;
    id.x = fp_zero(); id.y = fp_zero(); id.inf = true;
    ws_store_g1(ws, PL_P1X, BY_P1_INF, cbase + g, id);
  }
}
// One workgroup per (g, w): lane v loads bucket v's sum (the identity for an empty bucket and for v = 0), the fold of bn254_bitmap_rand.h
// runs in LDS (every addition in place there), and lane b < 8 writes T_{g, 8w + b} — affine, the identity flag carried — at its place among
// the group's table pairs, the key beside it.  A window without a contributor leaves at once.
KERNEL_FOLD void k_bmr_fold(Ws ws, BmrFold a) {
  const unsigned t = threadIdx.x;
  const size_t gw = blockIdx.x;
  const uint32_t mask = a.mask[gw];
  if (mask == 0) return;                               // the whole workgroup
  const uint64_t g = gw / a.nW;
  const uint32_t w = (uint32_t)(gw - g * a.nW);
  __shared__ BmrSlot B[BMR_FOLD_WG];
  __shared__ BmrSlot R[BMR_FOLD_WG / 2];
  __shared__ BmrSlot T[8];
  jac_set_identity(B[t].v);
  if (t != 0) {
    const uint64_t b = bmr_bucket(g, w, t, a.n_keys);
    if (a.cnt[b] != 0) {
      G1Affine p;
      ws_load_g1(ws, PL_P1X, BY_P1_INF, a.bpbase + a.tp[b] - 1, p);
      jac_from_affine(B[t].v, p);
    }
  }
  __syncthreads();
  for (int phase = 0; phase < BMR_FOLD_PHASES; ++phase) {
    bmr_fold_phase(B, R, T, phase, t);
    __syncthreads();
  }
  if (t >= 8 || !((mask >> t) & 1u)) return;
  G1Affine s;
  jac_to_affine(s, T[t].v);
  const size_t at = a.tbase + (gw ? a.tincl[gw - 1] : 0) + bmr_pair_rank(mask, t);
  ws_store_g1(ws, PL_P1X, BY_P1_INF, at, s);
  a.bkey[at] = 8u * w + t;
}

// ---- the exact aggregate key of the queued tuples -----------------------------------------------------------------------------------------
// k_bm_sum_pair (bn254_bitmap_pair.hip) over a device-side queue: lane pair e takes tuple map[e], e < *count; a workgroup past the queue
// leaves at once.  Rule 2 has run (a queued tuple's status is 0); the key goes to the Q planes at the tuple's index.
KERNEL_PAIR void k_bmr_sum_pair_q(const uint32_t* bits, size_t bm_words, BmKeys K, const int32_t* rec, const uint8_t* rec_inf, Ws ws, const uint32_t* map,
                                  const uint32_t* count) {
  const size_t q = *count;
  if ((size_t)blockIdx.x * (BN_PAIR_WG / 2) >= q) return;   // the whole workgroup
  const unsigned role = threadIdx.x & 1u;
  const size_t e = ((size_t)blockIdx.x * BN_PAIR_WG + threadIdx.x) >> 1;
  const bool live = e < q;
  const size_t i = live ? map[e] : 0;
  const uint32_t* row = bits + i * bm_words;
  __shared__ G2Jac lds_acc[BN_PAIR_WG];
  G2Jac& acc = lds_acc[threadIdx.x];
  if (rec) bm_sum_tables(acc, row, bm_words, live, K, rec, rec_inf);      // wave-uniform
  else bm_sum_keys(acc, row, bm_words, live, K);
  G2Affine pk;
  bm_sum_to_key(pk, acc);
  if (!live) return;
  ws_store_fp(ws, PL_QX0 + (int)role, i, pk.x.c[0]);
  ws_store_fp(ws, PL_QY0 + (int)role, i, pk.y.c[0]);
  if (role == 0) ws_byte(ws, BY_Q_INF, i) = pk.inf;
}

// (bn254_host.h) — also what the optimistic merge's fallback launches (bn254_merge.hip)
int launch_bitmap_sum_queued(bn254_ctx* c, hipStream_t s, const uint32_t* d_bits, size_t bm_words, size_t n, bool tables, const uint32_t* map,
                             const uint32_t* count) {
  const BmKeys Kb = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)c->n_keys};
  const int32_t* rec = tables ? (const int32_t*)c->bm_tab : nullptr;
  const uint8_t* rec_inf = tables ? c->bm_tab + ((c->n_keys + 7) / 8) * 256 * BM_REC_WORDS * sizeof(int32_t) : nullptr;
  k_bmr_sum_pair_q<<<(unsigned)((2 * n + BN_PAIR_WG - 1) / BN_PAIR_WG), BN_PAIR_WG, 0, s>>>(d_bits, bm_words, Kb, rec, rec_inf, c->ws, map, count);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// The sizes of a call (one slice): groups, buckets, sort elements, and the places in the workspace — tuples from 0 (sigma: P1, H(m): P2, the
// re-check's key: Q), the scaled points from ebase, the partial products of the group checks from pbase, the groups (S_g, their products)
// from cbase, the byte buckets' sums from bpbase, the table pairs from tbase.
struct BmrPlan {
  size_t n, G, ng, nW, nwin, Kv, n_b, n_e, n_gw, n_bp_max, n_tp_max, n_gslots, n_part, n_spart;
  int wg;
  size_t ebase, pbase, cbase, bpbase, tbase, ws_items, nb;
};
static BmrPlan bmr_plan(size_t n, size_t K, size_t bm_words, size_t group_tuples) {
  BmrPlan p = {};
  p.n = n;
  p.G = std::max<size_t>(group_tuples, 1);
  p.ng = (n + p.G - 1) / p.G;
  p.nW = (K + 7) / 8;
  p.nwin = std::min(4 * bm_words, p.nW);
  p.Kv = p.nW * BMR_WINDOW_BUCKETS;
  p.n_b = p.ng * (p.Kv + 1);
  p.n_e = (p.nwin + 1) * n;
  p.n_gw = p.ng * p.nW;
  p.n_bp_max = std::min(p.nwin * n, p.ng * p.Kv);
  p.n_tp_max = p.ng * std::min(K, 8 * p.nwin);
  p.wg = aggd_keyed_width(0, p.n_tp_max + p.ng);
  p.n_gslots = aggd_keyed_slots(p.wg, p.n_tp_max, p.ng);
  p.n_part = seg_partials(p.n_gslots, AGGD_WG_ELEMS);
  p.n_spart = seg_partials(p.n_e, AGGR_SUM_WG);
  p.ebase = aggd_round256(n);
  p.pbase = aggd_round256(p.ebase + 2 * n);
  p.cbase = aggd_round256(p.pbase + p.n_part);
  p.bpbase = aggd_round256(p.cbase + p.ng);
  p.tbase = aggd_round256(p.bpbase + p.n_bp_max);
  p.ws_items = p.tbase + p.n_tp_max;
  p.nb = (std::max(std::max(p.n_b, p.n_gw), n) + AGGD_SCAN_WG - 1) / AGGD_SCAN_WG;
  return p;
}
struct BmrScratch {
  uint64_t *cnt, *tp, *tincl, *glo, *ghi, *gkincl, *lo, *tot;
  uint32_t *nagg, *ebkt, *perm, *eseg, *mask, *bkey, *gseg0, *pseg, *spseg, *stats;
  int32_t* part;
  uint8_t *gst, *queued, *saved;
};
static BmrScratch bmr_scratch(Carve& c, const BmrPlan& p) {
  BmrScratch b;
  b.cnt = c.take<uint64_t>(p.n_b), b.tp = c.take<uint64_t>(p.n_b), b.tincl = c.take<uint64_t>(p.n_gw);
  b.glo = c.take<uint64_t>(p.ng), b.ghi = c.take<uint64_t>(p.ng), b.gkincl = c.take<uint64_t>(p.ng);
  b.lo = c.take<uint64_t>(p.n), b.tot = c.take<uint64_t>(p.nb);
  b.nagg = c.take<uint32_t>(p.ng);
  b.ebkt = c.take<uint32_t>(p.n_e), b.perm = c.take<uint32_t>(p.n_e), b.eseg = c.take<uint32_t>(p.n_e);
  b.mask = c.take<uint32_t>(p.n_gw);
  b.bkey = c.take<uint32_t>(p.tbase + p.n_tp_max);     // indexed by workspace position: a bucket's or a table pair's key beside its point
  b.gseg0 = c.take<uint32_t>(p.n_gslots);
  b.pseg = c.take<uint32_t>(p.n_part);
  b.spseg = c.take<uint32_t>(p.n_spart);
  b.stats = c.take<uint32_t>(8);                       // what bn254_debug_bitmap_rand_last reads
  b.part = c.take<int32_t>(AGGR_PART_WORDS * p.n_spart);
  b.gst = c.take<uint8_t>(p.ng), b.queued = c.take<uint8_t>(p.n), b.saved = c.take<uint8_t>(p.ng);
  return b;
}

// one slice on the randomised route; index_base = the slice's first tuple in the caller's arrays (r_i is numbered there)
static int bmr_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, const uint32_t* d_bits, size_t bm_words, size_t n,
                      uint32_t flags, const uint8_t* seed32, uint64_t index_base, uint8_t* d_status, hipStream_t s) {
  const size_t K = c->n_keys;
  const BmrPlan p = bmr_plan(n, K, bm_words, (size_t)c->bmr_group_tuples);
  Carve size(nullptr);
  bmr_scratch(size, p);
  int rc = ws_reserve(c, p.ws_items);
  if (rc || (rc = scratch_reserve(c, &c->bmr_buf, &c->bmr_cap, size.used))) return rc;
  Carve carve(c->bmr_buf);
  const BmrScratch b = bmr_scratch(carve, p);
  c->bmr_stats = b.stats;
  const KeyTable kt = {c->key_lines, c->key_st, c->key_inf, (uint32_t)K};
  BmrSeed seed;
  for (int j = 0; j < 8; ++j)
    seed.w[j] = ((uint32_t)seed32[4 * j] << 24) | ((uint32_t)seed32[4 * j + 1] << 16) | ((uint32_t)seed32[4 * j + 2] << 8) | seed32[4 * j + 3];
  const int mode = (flags & BN254_FLAG_RAND64) ? 1 : (flags & BN254_FLAG_RAND_GLV) ? 2 : 0;
  const uint32_t dflags = flags & ~(uint32_t)(BN254_FLAG_RAND64 | BN254_FLAG_RAND_GLV);
  CallDone call_done(c, s);
  const bool tables = bm_wants_tables(c);
  if ((rc = bm_prepare(c, s, tables))) return rc;      // the bad-bit vector for rule 2, the subset tables for the re-check
  c->bmr_last = {p.ng, p.cbase, p.tbase, b.nagg, b.bkey, b.glo, b.ghi, b.gst};   // nothing below rewrites these once the group checks are through
  const BmKeys Kb = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)K};
  PROF_MARK(0);                                        // ms[0] = sigma's decode + hash, ms[1] = statuses + ladders, ms[2] = sort, sums, fold, ms[3] = checks
  if ((rc = launch_decode_g1(c, s, d_sigs, n, dflags, PL_P1X, BY_P1_INF, 0))) return rc;
  if ((rc = launch_hash_rounds(c, s, d_msgs, d_off, n, PL_P2X, BY_P2_INF, nullptr))) return rc;
  PROF_MARK(1);
  HIP_TRY(hipMemsetAsync(b.nagg, 0, 4 * p.ng, s));
  HIP_TRY(hipMemsetAsync(b.cnt, 0, 8 * p.n_b, s));
  HIP_TRY(hipMemsetAsync(b.ebkt, 0xFF, 4 * p.n_e, s));
  HIP_TRY(hipMemsetAsync(b.eseg, 0xFF, 4 * p.n_e, s));
  k_bmr_status<<<grid_for(n), BN_WAVE, 0, s>>>(n, d_bits, bm_words, Kb, c->ws, (uint64_t)p.G, b.nagg, b.lo);
  const BmrScale sc = {b.nagg, b.ebkt, b.cnt, (uint64_t)p.G, index_base, p.ebase, (uint32_t)K, (uint32_t)p.nwin};
  k_bmr_scale<<<grid_for(2 * n), BN_WAVE, 0, s>>>(n, d_bits, bm_words, c->ws, sc, seed, mode);
  HIP_TRY(hipGetLastError());
  PROF_MARK(2);
  // the sort by bucket, the buckets' ranks, the places of the table pairs
  if ((rc = bn254_aggd_scan_add(s, b.cnt, p.n_b, b.tp, b.tot))) return rc;
  // b.tp serves twice, as in §10b's call: the scatter consumes it as its cursors, then (a later launch on the stream) the non-empty flags overwrite it
  if ((rc = bn254_aggr_scatter(p.n_e, b.ebkt, b.tp, b.perm, b.eseg, p.n_b, (uint32_t)p.Kv, b.cnt, b.tp, s))) return rc;
  k_bmr_perm_points<<<grid_for(p.n_e), BN_WAVE, 0, s>>>(p.n_e, n, (uint32_t)p.nwin, b.eseg, b.perm);
  if ((rc = bn254_aggd_scan_add(s, b.tp, p.n_b, b.tp, b.tot))) return rc;
  k_bmr_keymask<<<grid_for(p.n_gw), BN_WAVE, 0, s>>>(p.n_gw, (uint32_t)p.nW, (uint32_t)K, c->key_st, c->key_inf, b.cnt, b.mask, b.tincl);
  if ((rc = bn254_aggd_scan_add(s, b.tincl, p.n_gw, b.tincl, b.tot))) return rc;
  k_bmr_glimits<<<grid_for(p.ng), BN_WAVE, 0, s>>>(p.ng, (uint32_t)p.nW, (uint32_t)K, p.tbase, b.cnt, b.tincl, b.glo, b.ghi, c->ws, p.cbase);
  HIP_TRY(hipGetLastError());
  // the buckets' sums (S_g lands at cbase + g, a byte bucket's sum at bpbase + its rank), then the fold into the table pairs
  const AggrSum sm = {b.perm, b.tp, b.bkey, 0, p.ebase, p.cbase, p.bpbase, (uint32_t)p.Kv};
  size_t in = 0;
  seg_levels(p.n_e, AGGR_SUM_WG, [&](size_t e, size_t off, int last) {
    if (!rc) rc = bn254_aggr_sum(e, !off, c->ws, sm, off ? b.spseg + in : b.eseg, off ? b.part + AGGR_PART_WORDS * in : nullptr, b.spseg + off,
                                 b.part + AGGR_PART_WORDS * off, last, s);
    in = off;
  });
  if (rc) return rc;
  const BmrFold fo = {b.cnt, b.tp, b.tincl, b.mask, b.bkey, p.bpbase, p.tbase, (uint32_t)p.nW, (uint32_t)K};
  k_bmr_fold<<<(unsigned)p.n_gw, BMR_FOLD_WG, 0, s>>>(c->ws, fo);
  HIP_TRY(hipGetLastError());
  PROF_MARK(3);
  // one check per group: its table pairs and (S_g, -G2) through the slot kernel, the levels, the final exponentiation at index g — which
  // takes the status byte at g with it, a tuple's: those bytes step aside for it
  if ((rc = bn254_aggd_keyed_slot_map(s, p.ng, b.glo, b.ghi, p.wg, b.gkincl, b.tot, p.n_gslots, b.gseg0))) return rc;
  const AggdSlots gsl = {b.gseg0, b.gkincl, b.glo, b.ghi};
  in = 0;
  seg_levels(p.n_gslots, AGGD_WG_ELEMS, [&](size_t e, size_t off, int last) {
    if (!rc)
      rc = !off ? bn254_pair_aggd_keyed_queued(e, p.wg, c->ws, gsl, b.bkey, kt, p.cbase, p.pbase, b.pseg, last, nullptr, s)
                : bn254_pair_aggd_level(e, c->ws, b.pseg + in, p.pbase + in, p.cbase, p.pbase + off, b.pseg + off, last, s);
    in = off;
  });
  if (rc) return rc;
  uint8_t* st_bytes = c->ws.bytes + (size_t)BY_ST_DECODE * c->ws.stride;
  HIP_TRY(hipMemcpyAsync(b.saved, st_bytes, p.ng, hipMemcpyDeviceToDevice, s));
  if ((rc = bn254_pair_aggd_move(p.ng, c->ws, p.cbase, s))) return rc;
  if ((rc = launch_final_exp_layout(c, s, p.ng, 0, b.gst, route_for(c, p.ng).fe))) return rc;
  HIP_TRY(hipMemcpyAsync(st_bytes, b.saved, p.ng, hipMemcpyDeviceToDevice, s));
  // statuses; the tuples of failed groups (of two or more) queued and verified exactly — with none queued, launches that leave at once
  HIP_TRY(hipMemsetAsync(c->ws.h_cnt, 0, sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(c->bmr_stats, 0, 8 * sizeof(uint32_t), s));
  if ((rc = bn254_aggr_collect(n, c->ws, 0, b.lo, (uint64_t)p.G, b.nagg, b.gst, d_status, b.queued, p.ng, b.glo, b.ghi, c->bmr_stats, s))) return rc;
  if ((rc = launch_bitmap_sum_queued(c, s, d_bits, bm_words, n, tables, c->ws.h_list, c->ws.h_cnt))) return rc;
  if ((rc = bn254_pair_miller_verify(n, c->ws, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  if ((rc = bn254_pair_final_exp(n, c->ws, 1, d_status, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  c->bmr_last_ran = 1;                                 // only a call that enqueued everything has something for the debug hooks to read
  return 0;
}

// the checks of the exact call, the slicing, and the choice of route for a slice
static int bmr_call_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, const uint32_t* d_bits, size_t bm_words, size_t n,
                           uint32_t flags, const uint8_t* seed32, uint64_t index_base, uint8_t* d_status, void* stream) {
  const uint32_t dflags = flags & ~(uint32_t)(BN254_FLAG_RAND64 | BN254_FLAG_RAND_GLV);
  const size_t K = c->n_keys;
  // no keys, pair lanes off, too few tuples, too many keys: the exact call, same bytes.  Every slice comes through here, so the debug hooks speak of the last one.
  c->bmr_last_ran = 0;
  if (K == 0 || !c->key_lines || !c->pair_lanes || n < (size_t)c->bmr_min_tuples || K > (size_t)c->bmr_max_keys)
    return bn254_batch_verify_keyed_bitmap_device(c, d_msgs, d_off, d_sigs, d_bits, bm_words, n, dflags, d_status, stream);
  HIP_TRY(hipSetDevice(c->device));
  const size_t nW = (K + 7) / 8;
  if (const size_t chunk = ws_chunk_for(c, n, 4 + std::min(4 * bm_words, nW)))   // a slice is the same arrays further in; r_i keeps the caller's numbering
    return verify_device_sliced(n, chunk, [&](size_t lo, size_t len) {
      return bmr_call_device(c, d_msgs, d_off + lo, d_sigs + 64 * lo, d_bits ? d_bits + lo * bm_words : nullptr, bm_words, len, flags, seed32, index_base + lo,
                             d_status + lo, stream);
    });
  {  // buckets, sort elements and workspace entries are numbered in 32 bits: a piece beyond that takes the exact call too
    const BmrPlan p = bmr_plan(n, K, bm_words, (size_t)c->bmr_group_tuples);
    if (p.n_b > 0xFFFFFFF0u || p.n_e > 0xFFFFFFF0u || p.ws_items > 0xFFFFFFF0u)
      return bn254_batch_verify_keyed_bitmap_device(c, d_msgs, d_off, d_sigs, d_bits, bm_words, n, dflags, d_status, stream);
  }
  return bmr_device(c, d_msgs, d_off, d_sigs, d_bits, bm_words, n, flags, seed32, index_base, d_status, stream ? (hipStream_t)stream : c->stream);
}

extern "C" {

int bn254_batch_verify_keyed_bitmap_randomized_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs,
                                                      const uint32_t* d_bits, size_t bm_words, size_t n, uint32_t flags, const uint8_t* seed32,
                                                      uint8_t* d_status, void* stream) {
  if (g1c_flag(flags))                                  // compressed aggregates: staged once, in front of any slicing
    return g1c_call(c, d_sigs, n, n != 0, d_status, stream, [&](const uint8_t* d_sigs64) {
      return bn254_batch_verify_keyed_bitmap_randomized_device(c, d_msgs, d_off, d_sigs64, d_bits, bm_words, n, flags & ~BN254_FLAG_G1_COMPRESSED, seed32,
                                                               d_status, stream);
    });
  MsgsLenScope msgs_len_scope(c);
  if (!c || !seed32 || (n && (!d_msgs || !d_off || !d_sigs || !d_status || (bm_words && !d_bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  c->bmr_last_ran = 0;
  if (n == 0) return 0;
  if (misaligned(d_sigs) || misaligned(d_bits) || ((uintptr_t)d_off & 7u)) return BN254_E_MISALIGNED;
  return bmr_call_device(c, d_msgs, d_off, d_sigs, d_bits, bm_words, n, flags, seed32, 0, d_status, stream);
}

int bn254_batch_verify_keyed_bitmap_randomized(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, const uint32_t* bits,
                                               size_t bm_words, size_t n, uint32_t flags, const uint8_t* seed32, uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || !seed32 || (n && (!off || !sigs || !status || (bm_words && !bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  c->bmr_last_ran = 0;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, off, n)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)off[n]), *d_off = st.in(1, off, (n + 1) * sizeof(uint64_t));
  const uint8_t *d_sigs = st.in(2, sigs, n * g1_item_bytes(flags)), *d_bits = st.in(3, bits, n * bm_words * sizeof(uint32_t));
  uint8_t* d_status = st.out(4, n, status);
  if (st.ok())
    st.rc = bn254_batch_verify_keyed_bitmap_randomized_device(c, d_msgs, (const uint64_t*)d_off, d_sigs, (const uint32_t*)d_bits, bm_words, n, flags, seed32,
                                                              d_status, nullptr);
  return st.finish();
}

}  // extern "C"
