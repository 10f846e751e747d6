// Translation unit of libbn254hip.so: t-of-n threshold signatures over the registered keys and the segmented scalar-weighted sum in G1
// (include/bn254_hip.h: bn254_batch_threshold_combine_keyed[_device], bn254_batch_g1_msm[_device]).  The threshold call IS
// the exact collect (bn254_collect.hip: cl_collect_run, behind the family's shared checks and staging — bn254_host.h: ClCall: front end, range
// rule, keyed verify slices, claim pass) followed by rank-and-select on the rows it left, one Lagrange coefficient per kept key, and the
// term and sum kernels of the weighted sum.  The bookkeeping and the arithmetic are bn254_threshold.h and bn254_fr.h, shared with the CPU
// suite's host compilation.
// bn254_batch_threshold_combine_keyed_optimistic[_device] interpolates first — candidate rows from the optimistic collect's
// pre-check, the `threshold` lowest candidates, the same coefficient, term and sum kernels under a gate — and verifies each tuple's result
// ONCE under the group key (bn254_ctx_set_group_key: a one-entry key table, through the keyed verify's routing); only the tuples that fail,
// name a key twice or have too few candidates send their candidates through the collect's queue into the exact keyed kernels and are
// settled and interpolated again (th_combine_opt_device).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/bn254_hip.h"
#include "bn254_hash.h"
#include "bn254_io.h"
#include "bn254_pairing.h"
#include "bn254_collect.h"
#include "bn254_fr.h"
#include "bn254_threshold.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"
#include "bn254_aggd_plan.h"

// per term: the ladder's Jacobian result and the point's decode status; for the threshold call also, per share, the coefficient (32 B
// big-endian) and the take flag, and per tuple the second claim row
struct ThScratch { G1Jac* terms; uint32_t* claim; uint8_t *scalars, *mask, *term_st; };
static ThScratch th_scratch(Carve& c, size_t items, size_t claim_words, bool coefficients) {
  ThScratch b;
  b.terms = c.take<G1Jac>(items);
  b.claim = c.take<uint32_t>(claim_words);
  b.scalars = (uint8_t*)c.take<uint32_t>(coefficients ? items * 8 : 0);
  b.mask = c.take<uint8_t>(coefficients ? items : 0);
  b.term_st = c.take<uint8_t>(items);
  return b;
}
// ... and behind them, for the optimistic call: key index 0 for every slot of a piece of the tuple check, and per tuple the duplicate byte of
// the candidate rows and the gate of the interpolation now running
struct ThOptScratch { uint32_t* zeros; uint8_t *dup, *gate; };
static ThOptScratch th_opt_scratch(Carve& c, size_t n, size_t t_piece) {
  ThOptScratch b;
  b.zeros = c.take<uint32_t>(t_piece);
  b.dup = c.take<uint8_t>(n), b.gate = c.take<uint8_t>(n);
  return b;
}
// opt_piece != 0: the optimistic call of n tuples, its tuple check in pieces of opt_piece
static int th_scratch_reserve(bn254_ctx* c, size_t items, size_t claim_words, bool coefficients, ThScratch* T, size_t n = 0, size_t opt_piece = 0,
                              ThOptScratch* O = nullptr) {
  Carve size(nullptr);
  th_scratch(size, items, claim_words, coefficients);
  if (O) th_opt_scratch(size, n, opt_piece);
  if (const int rc = scratch_reserve(c, &c->th_buf, &c->th_cap, size.used)) return rc;
  Carve carve(c->th_buf);
  *T = th_scratch(carve, items, claim_words, coefficients);
  if (O) *O = th_opt_scratch(carve, n, opt_piece);
  return 0;
}

// ---- the weighted sum ------------------------------------------------------------------------------------------------------------------------------
// one lane per term.  No early return: the ladder's additions vote across the wave; a lane past the end, or masked out, walks the identity,
// and a wave with no term to take leaves at once (bn254_threshold.h: msm_term).
KERNEL void k_msm_term(const uint8_t* pts, const uint8_t* scalars, const uint8_t* mask, size_t m, int reduce, G1Jac* terms, uint8_t* term_st) {
  const size_t s = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = s < m, take = live && (!mask || mask[s] != 0);
  G1Jac t;
  uint8_t st = ST_OK;
  if (BN_WAVE_ANY(take)) msm_term(t, st, pts + 64 * (take ? s : 0), scalars + 32 * (take ? s : 0), reduce != 0, take);
  else jac_set_identity(t);
  if (!live) return;
  terms[s] = t;
  term_st[s] = st;
}
// lane per segment, the segments below wave_min terms (and the refused ones, which have none); wave per segment, the others — the layouts
// of k_cl_sum_lane / k_cl_sum_wave.  status == nullptr: the threshold call, whose statuses stand already.
KERNEL_SMALL void k_msm_sum_lane(const G1Jac* terms, const uint8_t* term_st, const uint64_t* seg, uint64_t m, const uint8_t* gate, size_t n, uint64_t wave_min,
                                 uint8_t* out, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  uint8_t seg_st = MSM_SEG_MASKED;
  uint64_t len = live ? msm_seg_len(seg, i, m, gate, seg_st) : 0;
  const bool mine = live && seg_st != MSM_SEG_MASKED && (seg_st != ST_OK || len < wave_min);
  if (!mine) len = 0;
  G1Jac acc;
  uint8_t st = ST_OK;
  msm_lane_sum(acc, st, terms, term_st, len ? seg[i] : 0, len);
  if (mine && seg_st != ST_OK) st = seg_st;
  G1Affine r;
  jac_to_affine(r, acc);
  if (!mine) return;
  if (st != ST_OK) r.inf = true;
  encode_g1(out + 64 * i, r);
  if (status) status[i] = st;
}
KERNEL_SMALL void k_msm_sum_wave(const G1Jac* terms, const uint8_t* term_st, const uint64_t* seg, uint64_t m, const uint8_t* gate, size_t n, uint64_t wave_min,
                                 uint8_t* out, uint8_t* status) {
  __shared__ ClJacSlot part[BN_WAVE];
  __shared__ uint32_t cnt[BN_WAVE];
  __shared__ uint64_t bad[BN_WAVE];
  __shared__ uint8_t st[BN_WAVE];
  const unsigned t = threadIdx.x;
  for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
    uint8_t seg_st;
    const uint64_t len = msm_seg_len(seg, i, m, gate, seg_st);
    if (seg_st != ST_OK || len < wave_min) continue;   // wave-uniform
    msm_wave_partial(part[t].v, st[t], bad[t], terms, term_st, seg[i], len, t);
    cnt[t] = 1;
    __syncthreads();
    for (unsigned stride = BN_WAVE / 2; stride >= 1; stride >>= 1) {
      if (t < stride) msm_tree_level(part, cnt, st, bad, t, stride);
      __syncthreads();
    }
    if (t == 0) {
      msm_encode(out + 64 * i, part[0].v, st[0]);
      if (status) status[i] = st[0];
    }
    __syncthreads();
  }
}
// terms and sums of m terms in n segments, enqueued on s; T holds m terms.  mask / gate: the threshold call's take flags and tuple statuses.
static int launch_msm(bn254_ctx* c, hipStream_t s, const uint8_t* d_points, const uint8_t* d_scalars, const uint8_t* d_mask, size_t m, const uint64_t* d_seg,
                      const uint8_t* d_gate, size_t n, int reduce, const ThScratch& T, uint8_t* d_out, uint8_t* d_status) {
  if (m) {
    k_msm_term<<<grid_for(m), BN_WAVE, 0, s>>>(d_points, d_scalars, d_mask, m, reduce, T.terms, T.term_st);
    HIP_TRY(hipGetLastError());
  }
  const uint64_t wave_min = (uint64_t)c->collect_wave_min;
  k_msm_sum_lane<<<grid_for(n), BN_WAVE, 0, s>>>(T.terms, T.term_st, d_seg, (uint64_t)m, d_gate, n, wave_min, d_out, d_status);
  HIP_TRY(hipGetLastError());
  k_msm_sum_wave<<<(unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS), BN_WAVE, 0, s>>>(T.terms, T.term_st, d_seg, (uint64_t)m, d_gate, n, wave_min, d_out,
                                                                                               d_status);
  HIP_TRY(hipGetLastError());
  return 0;
}
// the _device form behind its argument checks, the number of terms known
static int msm_device(bn254_ctx* c, const uint8_t* d_points, const uint8_t* d_scalars, const uint64_t* d_seg, size_t m, size_t n, int reduce, uint8_t* d_out,
                      uint8_t* d_status, hipStream_t s) {
  if (m > 0xFFFFFFFFu || (m && (!d_points || !d_scalars))) return BN254_E_BAD_ARGUMENT;
  ThScratch T;
  if (const int rc = th_scratch_reserve(c, m, 0, false, &T)) return rc;
  CallDone call_done(c, s);
  return launch_msm(c, s, d_points, d_scalars, nullptr, m, d_seg, nullptr, n, reduce, T, d_out, d_status);
}

// ---- the threshold call behind the collect -------------------------------------------------------------------------------------------------------
// lane per tuple: |V| against the threshold, the row cut down to S or the tuple failed (bn254_threshold.h: th_settle)
KERNEL_SMALL void k_th_settle(size_t n, size_t bm_words, uint32_t threshold, uint32_t* used, uint8_t* tuple_st, uint8_t* sigs, uint32_t* n_valid) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  uint8_t st = tuple_st[i];
  const uint32_t count = th_settle(used + i * bm_words, bm_words, threshold, st, sigs + 64 * i);
  tuple_st[i] = st;
  if (n_valid) n_valid[i] = count;
}
// lane per share: the one summand of every kept key claims it and writes the key's coefficient
KERNEL_SMALL void k_th_coeff(ClShares in, size_t n_shares, size_t n, size_t bm_words, const uint64_t* end, const uint32_t* used, uint32_t* claim, uint8_t* scalars,
                             uint8_t* mask) {
  const size_t s = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (s >= n_shares) return;
  const size_t t = cl_tuple_of(s, end, in.off, n);
  const bool take = th_take(in, s, t, n, used, claim, bm_words);
  mask[s] = take ? 1 : 0;
  if (take) fr_to_be(scalars + 32 * s, th_lagrange_row(used + t * bm_words, bm_words, in.key[s]));
}

// the call's outputs under the collect's names: agg_sigs = the group signatures, signer_bits = the rows of the keys used, n_signers = the counts
// of keys with a valid share
static int th_combine_device(bn254_ctx* c, const ClCall& a, uint32_t threshold, void* stream) {
  if (g1c_flag(a.flags))                                // compressed shares: staged once, in front of the collect and of the interpolation
    return cl_g1c_call(c, a, stream, [&](const ClCall& d) { return th_combine_device(c, d, threshold, stream); });
  MsgsLenScope msgs_len_scope(c);
  int rc = BN254_E_BAD_ARGUMENT;
  if (threshold == 0 || !cl_keys_ok(c, a) || !cl_checks_device(c, a, &rc)) return rc;
  const size_t n = a.n, n_shares = a.n_items, bm_words = a.bm_words;
  // this call's scratch before the first kernel (growing it waits for the context's streams); the collect reserves its own the same way
  ThScratch T;
  if ((rc = th_scratch_reserve(c, n_shares, n * bm_words, true, &T))) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  // 1. the exact collect behind its checks: share statuses, tuple statuses (2, or the hash's), row V, and the plain sum where the group
  // signature will go — no counts, which are step 2's; S: the scratch it carved, for the share -> tuple search
  c->clr_last_ran = c->clo_last_ran = c->mgo_last_ran = c->tho_last_ran = 0;
  ClCall collect = a;
  collect.n_signers = nullptr;
  ClScratch S;
  if ((rc = cl_collect_run(c, collect, nullptr, false, s, &S))) return rc;
  // 2. rank and select; 3. one coefficient per kept key, at the share that claims it; 4. terms and sums over the kept shares
  k_th_settle<<<grid_for(n), BN_WAVE, 0, s>>>(n, bm_words, threshold, a.signer_bits, a.tuple_status, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  if (n * bm_words) HIP_TRY(hipMemsetAsync(T.claim, 0, n * bm_words * sizeof(uint32_t), s));
  const ClShares in = {a.items, a.aux, a.off, a.item_status, a.tuple_status};
  if (n_shares) {
    k_th_coeff<<<grid_for(n_shares), BN_WAVE, 0, s>>>(in, n_shares, n, bm_words, S.end, a.signer_bits, T.claim, T.scalars, T.mask);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = launch_msm(c, s, a.items, T.scalars, T.mask, n_shares, a.off, a.tuple_status, n, 0, T, a.agg_sigs, nullptr))) return rc;
  PROF_MARK(0);                                        // the collect's layout (EV_COLLECT): ms[1] = its select-and-sum and the interpolation
  return 0;
}

// ---- the optimistic call: interpolate first, verify the result once per tuple under the group key ---------------------------
// lane per share: a candidate (status 0, of an accepted tuple) claims its key's bit in its tuple's row.  flag == nullptr: the first pass, over
// the pre-check statuses, a refused claim raising the tuple's duplicate byte; else the second pass, over the verified statuses of the tuples
// that go the exact way, whose rows k_clo_settle zeroed (which of several valid shares of a key claims does not matter: bn254_collect.h)
KERNEL_SMALL void k_tho_rows(size_t n_shares, size_t n, size_t bm_words, const uint32_t* key, const uint64_t* off, const uint64_t* end,
                             const uint8_t* share_st, const uint8_t* flag, const uint8_t* verdict, uint32_t* rows, uint8_t* dup) {
  const size_t s = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (s >= n_shares || share_st[s] != ST_OK) return;
  const size_t t = cl_tuple_of(s, end, off, n);
  if (t >= n) return;
  uint8_t ignored = 0;
  if (!flag) tho_candidate(rows + t * bm_words, bm_words, key[s], dup + t);
  else if (tho_reclaims(share_st[s], t, n, flag, verdict)) tho_candidate(rows + t * bm_words, bm_words, key[s], &ignored);
}
// lane per tuple behind the candidate rows: the tuple's flag, S' or the zeroed signature, the count of candidates, the first gate
KERNEL_SMALL void k_tho_settle(size_t n, size_t bm_words, uint32_t threshold, const uint8_t* tuple_st, const uint8_t* dup, uint32_t* used, uint8_t* sigs,
                               uint32_t* n_valid, uint8_t* flag, uint8_t* gate) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  uint32_t count;
  const uint8_t f = tho_settle(used + i * bm_words, bm_words, threshold, tuple_st[i], dup[i], sigs + 64 * i, count);
  flag[i] = f;
  gate[i] = tho_gate(f);
  if (n_valid) n_valid[i] = count;
}
// lane per tuple behind the second claim pass: the tuples that went the exact way settled as the exact call settles them, the second gate
KERNEL_SMALL void k_tho_resettle(size_t n, size_t bm_words, uint32_t threshold, const uint8_t* flag, const uint8_t* verdict, uint32_t* used, uint8_t* tuple_st,
                                 uint8_t* sigs, uint32_t* n_valid, uint8_t* gate) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  uint8_t st = tuple_st[i];
  uint32_t count = 0;
  bool mine;
  gate[i] = tho_resettle(used + i * bm_words, bm_words, threshold, flag[i], verdict[i], st, sigs + 64 * i, count, mine);
  if (!mine) return;
  tuple_st[i] = st;
  if (n_valid) n_valid[i] = count;
}
// one interpolation under a gate: a coefficient per kept key of the tuples the gate lets through, then terms and sums — the exact call's kernels
static int th_interpolate(bn254_ctx* c, hipStream_t s, const ClCall& a, const ClScratch& S, const ThScratch& T, const uint8_t* gate) {
  const size_t n = a.n, n_shares = a.n_items, bm_words = a.bm_words;
  if (n * bm_words) HIP_TRY(hipMemsetAsync(T.claim, 0, n * bm_words * sizeof(uint32_t), s));
  const ClShares in = {a.items, a.aux, a.off, a.item_status, gate};
  if (n_shares) {
    k_th_coeff<<<grid_for(n_shares), BN_WAVE, 0, s>>>(in, n_shares, n, bm_words, S.end, a.signer_bits, T.claim, T.scalars, T.mask);
    HIP_TRY(hipGetLastError());
  }
  return launch_msm(c, s, a.items, T.scalars, T.mask, n_shares, a.off, gate, n, 0, T, a.agg_sigs, nullptr);
}
static int th_combine_opt_device(bn254_ctx* c, const ClCall& a, uint32_t threshold, void* stream) {
  if (g1c_flag(a.flags))                                // compressed shares: staged once, whichever route the call takes
    return cl_g1c_call(c, a, stream, [&](const ClCall& d) { return th_combine_opt_device(c, d, threshold, stream); });
  // no group key: nothing to check the result against — whatever route the call would take
  if (threshold == 0 || !c || !c->gk_set) return BN254_E_BAD_ARGUMENT;
  // WHOLE-CALL ROUTING: the exact call (same bytes) for a call too small to pay, for an empty key set and without the lane-pair kernels
  if (!a.n_items || a.n_items < (size_t)c->th_opt_min_shares || !c->n_keys || !c->key_lines || !c->pair_lanes) return th_combine_device(c, a, threshold, stream);
  MsgsLenScope msgs_len_scope(c);
  int rc = BN254_E_BAD_ARGUMENT;
  if (!cl_keys_ok(c, a) || !cl_checks_device(c, a, &rc)) return rc;
  const size_t n = a.n, n_shares = a.n_items, bm_words = a.bm_words;
  c->clr_last_ran = c->clo_last_ran = c->mgo_last_ran = c->tho_last_ran = 0;
  // every buffer before the first kernel (growing one waits for the context's streams): the workspace of the longest piece — tuples for the
  // hash and the tuple check, shares for the queue — the collect family's scratch, and this call's own
  const size_t t_chunk = ws_chunk_for(c, n), s_chunk = ws_chunk_for(c, n_shares);
  const size_t t_piece = t_chunk ? t_chunk : n, s_piece = s_chunk ? s_chunk : n_shares;
  if ((rc = ws_reserve(c, t_piece > s_piece ? t_piece : s_piece))) return rc;
  ClScratch S;
  if ((rc = cl_scratch_reserve(c, n, &S))) return rc;
  ThScratch T;
  ThOptScratch O;
  if ((rc = th_scratch_reserve(c, n_shares, n * bm_words, true, &T, n, t_piece, &O))) return rc;
  c->tho_stats = S.stats + CLO_STAT_AT;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  const KeyTable gk = {c->gk_lines, c->gk_st, c->gk_inf, 1u};
  HIP_TRY(hipMemsetAsync(S.stats, 0, CL_STAT_WORDS * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(O.zeros, 0, t_piece * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(O.dup, 0, n, s));
  PROF_MARK(0);
  // 1. the front end of the family: hash once per tuple, the range rule, the fills; rules 1-3 of every share; the candidate rows
  if ((rc = cl_hash_and_plan(c, s, a, t_piece, S))) return rc;
  if (bm_words) HIP_TRY(hipMemsetAsync(a.signer_bits, 0, n * bm_words * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(a.item_status, ST_INDEX_OOB, n_shares, s));
  if ((rc = clo_precheck_all(c, s, a, S))) return rc;
  k_tho_rows<<<grid_for(n_shares), BN_WAVE, 0, s>>>(n_shares, n, bm_words, a.aux, a.off, S.end, a.item_status, nullptr, nullptr, a.signer_bits, O.dup);
  HIP_TRY(hipGetLastError());
  // 2. per tuple: final, the exact way at once, or S' = the lowest `threshold` candidates; 3. the interpolation over S'
  k_tho_settle<<<grid_for(n), BN_WAVE, 0, s>>>(n, bm_words, threshold, a.tuple_status, O.dup, a.signer_bits, a.agg_sigs, a.n_signers, S.flag, O.gate);
  HIP_TRY(hipGetLastError());
  PROF_MARK(1);
  if ((rc = th_interpolate(c, s, a, S, T, O.gate))) return rc;
  // 4. the tuple check under the group key: key index 0 of its one-entry table for every slot, the signatures decoded with flags 0
  for (size_t lo = 0; lo < n; lo += t_piece) {
    const size_t len = n - lo < t_piece ? n - lo : t_piece;
    if ((rc = launch_decode_g1(c, s, a.agg_sigs + 64 * lo, len, 0, PL_P1X, BY_P1_INF, 0))) return rc;
    if ((rc = clo_load_h(c, s, lo, len, S))) return rc;
    PROF_MARK(2);
    if ((rc = launch_keyed_miller_fe(c, s, len, O.zeros, S.verdict + lo, gk, c->gk_xy))) return rc;
  }
  PROF_MARK(3);
  // 5. / 6. the verdicts counted and the rows of the tuples that go the exact way zeroed; their candidates verified one by one through the
  // queue; their rows claimed again from the verified statuses, settled as the exact call settles them, and interpolated again
  if ((rc = clo_settle(c, s, a, S))) return rc;
  const KeyTable kt = ctx_key_table(c);
  for (size_t lo = 0; lo < n_shares; lo += s_piece) {
    const size_t len = n_shares - lo < s_piece ? n_shares - lo : s_piece;
    if ((rc = clo_queue_slice(c, s, a, lo, len, S))) return rc;
    if ((rc = bn254_pair_miller_verify_keyed(len, c->ws, a.aux + lo, kt, s, 0, c->ws.h_list, c->ws.h_cnt))) return rc;
    if ((rc = bn254_pair_final_exp(len, c->ws, 1, a.item_status + lo, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  }
  k_tho_rows<<<grid_for(n_shares), BN_WAVE, 0, s>>>(n_shares, n, bm_words, a.aux, a.off, S.end, a.item_status, S.flag, S.verdict, a.signer_bits, O.dup);
  HIP_TRY(hipGetLastError());
  k_tho_resettle<<<grid_for(n), BN_WAVE, 0, s>>>(n, bm_words, threshold, S.flag, S.verdict, a.signer_bits, a.tuple_status, a.agg_sigs, a.n_signers, O.gate);
  HIP_TRY(hipGetLastError());
  if ((rc = th_interpolate(c, s, a, S, T, O.gate))) return rc;
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  c->tho_last_ran = 1;
  return 0;
}

extern "C" {

int bn254_batch_g1_msm_device(bn254_ctx* c, const uint8_t* d_points, const uint8_t* d_scalars, const uint64_t* d_seg_off, size_t n, int reduce_scalar,
                              uint8_t* d_out, uint8_t* d_status, void* stream) {
  if (!c || n > 0xFFFFFFFFu || (n && (!d_seg_off || !d_out || !d_status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_points) || misaligned(d_scalars) || misaligned(d_out) || ((uintptr_t)d_seg_off & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the number of terms is d_seg_off[n], which sizes the scratch: one 8-byte copy home and a wait for the stream (include/bn254_hip.h)
  uint64_t m = 0;
  HIP_TRY(hipMemcpyAsync(&m, d_seg_off + n, sizeof m, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return msm_device(c, d_points, d_scalars, d_seg_off, (size_t)m, n, reduce_scalar, d_out, d_status, s);
}
int bn254_batch_g1_msm(bn254_ctx* c, const uint8_t* points, const uint8_t* scalars, const uint64_t* seg_off, size_t n, int reduce_scalar, uint8_t* out,
                       uint8_t* status) {
  if (!c || n > 0xFFFFFFFFu || (n && (!seg_off || !out || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!offsets_ok(seg_off, n)) return BN254_E_BAD_ARGUMENT;
  const size_t total = (size_t)seg_off[n];
  if (total && (!points || !scalars)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_points = st.in(0, points, total * 64), *d_scalars = st.in(1, scalars, total * 32), *d_seg = st.in(2, seg_off, (n + 1) * sizeof(uint64_t));
  uint8_t *d_out = st.out(3, n * 64, out), *d_status = st.out(4, n, status);
  if (st.ok()) st.rc = msm_device(c, d_points, d_scalars, (const uint64_t*)d_seg, total, n, reduce_scalar, d_out, d_status, c->stream);
  return st.finish();
}

int bn254_batch_threshold_combine_keyed_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_shares,
                                               const uint32_t* d_share_key, const uint64_t* d_share_off, size_t n_shares, size_t n, size_t bm_words,
                                               uint32_t threshold, uint32_t flags, uint8_t* d_share_status, uint8_t* d_tuple_status, uint8_t* d_group_sigs,
                                               uint32_t* d_used_bits, uint32_t* d_n_valid, void* stream) {
  const ClCall a = {.msgs = d_msgs, .msg_off = d_msg_off, .items = d_shares, .aux = d_share_key, .off = d_share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = d_share_status, .tuple_status = d_tuple_status, .agg_sigs = d_group_sigs,
                    .signer_bits = d_used_bits, .n_signers = d_n_valid};
  return th_combine_device(c, a, threshold, stream);
}
// the host-pointer form: the checks and the staging of the collect's (bn254_collect.hip: cl_collect_host), the five outputs in slot 5
int bn254_batch_threshold_combine_keyed(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* shares, const uint32_t* share_key,
                                        const uint64_t* share_off, size_t n_shares, size_t n, size_t bm_words, uint32_t threshold, uint32_t flags,
                                        uint8_t* share_status, uint8_t* tuple_status, uint8_t* group_sigs, uint32_t* used_bits, uint32_t* n_valid) {
  const ClCall a = {.msgs = msgs, .msg_off = msg_off, .items = shares, .aux = share_key, .off = share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = share_status, .tuple_status = tuple_status, .agg_sigs = group_sigs,
                    .signer_bits = used_bits, .n_signers = n_valid};
  MsgsLenScope msgs_len_scope(c);
  int rc = BN254_E_BAD_ARGUMENT;
  if (threshold == 0 || !cl_keys_ok(c, a) || !cl_checks_host(c, a, &rc)) return rc;
  HostStaging st(c);
  ClCall d;
  cl_stage(st, a, 1, 5, &d);
  if (st.ok()) st.rc = th_combine_device(c, d, threshold, nullptr);
  return st.finish();
}

int bn254_batch_threshold_combine_keyed_optimistic_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_shares,
                                                          const uint32_t* d_share_key, const uint64_t* d_share_off, size_t n_shares, size_t n,
                                                          size_t bm_words, uint32_t threshold, uint32_t flags, uint8_t* d_share_status,
                                                          uint8_t* d_tuple_status, uint8_t* d_group_sigs, uint32_t* d_used_bits, uint32_t* d_n_valid,
                                                          void* stream) {
  const ClCall a = {.msgs = d_msgs, .msg_off = d_msg_off, .items = d_shares, .aux = d_share_key, .off = d_share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = d_share_status, .tuple_status = d_tuple_status, .agg_sigs = d_group_sigs,
                    .signer_bits = d_used_bits, .n_signers = d_n_valid};
  return th_combine_opt_device(c, a, threshold, stream);
}
int bn254_batch_threshold_combine_keyed_optimistic(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* shares,
                                                   const uint32_t* share_key, const uint64_t* share_off, size_t n_shares, size_t n, size_t bm_words,
                                                   uint32_t threshold, uint32_t flags, uint8_t* share_status, uint8_t* tuple_status,
                                                   uint8_t* group_sigs, uint32_t* used_bits, uint32_t* n_valid) {
  const ClCall a = {.msgs = msgs, .msg_off = msg_off, .items = shares, .aux = share_key, .off = share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = share_status, .tuple_status = tuple_status, .agg_sigs = group_sigs,
                    .signer_bits = used_bits, .n_signers = n_valid};
  MsgsLenScope msgs_len_scope(c);
  int rc = BN254_E_BAD_ARGUMENT;
  if (threshold == 0 || !c || !c->gk_set || !cl_keys_ok(c, a) || !cl_checks_host(c, a, &rc)) return rc;
  HostStaging st(c);
  ClCall d;
  cl_stage(st, a, 1, 5, &d);
  if (st.ok()) st.rc = th_combine_opt_device(c, d, threshold, nullptr);
  return st.finish();
}

}  // extern "C"
