// Translation unit of libbn254hip.so: merging partial signer-bitmap aggregates into one aggregate per message (include/bn254_hip.h:
// bn254_batch_merge_keyed_bitmap[_device]) — the inner node of an aggregation tree.  The front end is the collect's
// (bn254_collect.hip: hash once per tuple, range rule, spread of H(m) over the tuple's partials), the verify of a slice of partials is the
// bitmap verify's (bn254_bitmap.hip: bm_prepare, launch_bitmap_sum; launch_verify_miller_fe), and the first-fit select-and-sum in two
// layouts is this unit's; its walk and arithmetic are bn254_merge.h, shared with the CPU suite's host compilation.
// bn254_batch_merge_keyed_bitmap_optimistic[_device] verifies each tuple's provisional SUM once, by the same kernels, and
// sends only the candidates of the tuples that fail — or hold an overlap — through a device-side queue into the bitmap verify's lane-pair
// kernels (mg_optimistic).
// Per-partial semantics: ECDSA::verify (/root/reference/src/ecdsa.rs:49-64) against the sum of the selected keys (`Add for PublicKey`,
// src/types.rs:126-132); the sum: `Add for Signature` (src/types.rs:264-270).
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
#include "bn254_merge.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"

// ---- select-and-sum (both kernels run on the zeroed output rows and the zeroed part_taken; a tuple is taken by exactly one of them, by its
// own number of partials) ---------------------------------------------------------------------------------------------------------------------
// lane per tuple, the tuples below wave_min partials.  No early return: the additions vote across the wave (see k_cl_sum_lane); a lane whose
// tuple is long, or past the end, walks identities.
KERNEL_SMALL void k_mg_lane(MgParts in, size_t n, size_t bm_words, uint64_t wave_min, uint8_t* part_taken, uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  uint64_t len = mg_tuple_len(in, live ? i : 0, live);
  const bool mine = live && len < wave_min;
  if (!mine) len = 0;
  G1Jac acc;
  uint32_t count;
  mg_lane_walk(acc, count, bits + (mine ? i : 0) * bm_words, part_taken, bm_words, in, mine ? in.off[i] : 0, len);
  G1Affine r;
  jac_to_affine(r, acc);
  if (!mine) return;
  encode_g1(agg + 64 * i, r);
  if (n_signers) n_signers[i] = count;
}
// wave per tuple, the others: a wave leaves a short tuple at once (wave-uniformly); tuples beyond the grid by stride.  Select first — lane l
// owns words l, l + 64, .. of the row, lane 0 writes part_taken —, a barrier (the sum reads part_taken as other lanes' stores left it), the
// partial sums accumulated in place in LDS as k_cl_sum_wave keeps them, the collect's tree, and the popcount of the row beside it.
KERNEL_SMALL void k_mg_wave(MgParts in, size_t n, size_t bm_words, uint64_t wave_min, uint8_t* part_taken, uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  __shared__ ClJacSlot part[BN_WAVE];
  __shared__ uint32_t cnt[BN_WAVE];
  const unsigned t = threadIdx.x;
  for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t len = mg_tuple_len(in, i, true);
    if (len < wave_min) continue;
    uint32_t* row = bits + i * bm_words;
    mg_wave_select(row, part_taken, bm_words, in, in.off[i], len, t);
    __syncthreads();
    mg_wave_partial(part[t].v, cnt[t], row, part_taken, bm_words, in, in.off[i], len, t);
    __syncthreads();
    for (unsigned stride = BN_WAVE / 2; stride >= 1; stride >>= 1) {
      if (t < stride) cl_tree_level(part, cnt, t, stride);
      __syncthreads();
    }
    if (t == 0) {
      cl_encode(agg + 64 * i, part[0].v);
      if (n_signers) n_signers[i] = cnt[0];
    }
    __syncthreads();
  }
}

// one slice of the partials: decode, spread, the aggregate keys of the slice's rows (rule 2 behind the decode status; a partial of no tuple
// keeps the 2 the spread gave it), the verify; statuses at the partials' own positions.  Profiling: every slice records its intervals, so the
// last one's stay, as in the collect.
static int mg_verify_slice(bn254_ctx* c, hipStream_t s, const uint8_t* d_parts, const uint32_t* d_part_bits, const uint64_t* d_part_off, size_t n, size_t lo,
                           size_t len, size_t bm_words, uint32_t flags, bool tables, const ClScratch& S, uint8_t* d_part_status) {
  int rc;
  if (lo) PROF_MARK(1);
  if ((rc = launch_decode_g1(c, s, d_parts + 64 * lo, len, flags, PL_P1X, BY_P1_INF, 0))) return rc;
  if ((rc = launch_cl_spread(c, s, len, (uint64_t)lo, n, d_part_off, S))) return rc;
  if ((rc = launch_bitmap_sum(c, s, d_part_bits ? d_part_bits + lo * bm_words : nullptr, bm_words, len, tables))) return rc;
  PROF_MARK(2);
  if ((rc = launch_verify_miller_fe(c, s, len, BN_PAIRS_VERIFY, 1, d_part_status + lo, true))) return rc;
  PROF_MARK(4);
  return 0;
}

// ---- the optimistic route (the steps are bn254_merge.h's mgo_*) ---------------------------------------------------------------
// rules 1-3 of every partial of an accepted tuple, straight from the caller's bytes: no workspace, no pairing, no aggregate key.  A partial of
// nobody keeps the 2 the status array was filled with.
KERNEL_SMALL void k_mgo_precheck(size_t n_parts, size_t n, const uint8_t* parts, const uint32_t* rows, const uint64_t* off, size_t bm_words, uint32_t flags,
                                 ClScratch S, BmKeys K, uint8_t* part_status) {
  const size_t p = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (p >= n_parts) return;
  const size_t t = cl_tuple_of(p, S.end, off, n);
  if (t >= n) return;
  part_status[p] = mgo_precheck(parts + 64 * p, flags, rows + p * bm_words, bm_words, K, S.hst[t]);
}
// k_mg_lane / k_mg_wave with the candidates counted and a refused candidate reported.  verdict == nullptr: the PROVISIONAL select-and-sum of
// every tuple over the pre-check statuses, which also writes the tuple's flag; else the RE-SELECT of the tuples that go the exact way (their
// rows zeroed by k_mgo_settle) over the final statuses — a tuple that does not go the exact way has length 0 and nothing of it is written.
KERNEL_SMALL void k_mgo_lane(MgParts in, size_t n, size_t bm_words, uint64_t wave_min, const uint8_t* verdict, uint8_t* flag, uint8_t* part_taken,
                             uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  uint64_t len = verdict ? mgo_resum_len(in, live ? i : 0, live, flag, verdict) : mg_tuple_len(in, live ? i : 0, live);
  const bool mine = live && len < wave_min && (!verdict || clo_goes_exact(flag[i], verdict[i]));
  if (!mine) len = 0;
  G1Jac acc;
  uint32_t count, cand, overlap;
  mgo_lane_walk(acc, count, cand, overlap, bits + (mine ? i : 0) * bm_words, part_taken, bm_words, in, mine ? in.off[i] : 0, len);
  G1Affine r;
  jac_to_affine(r, acc);
  if (!mine) return;
  encode_g1(agg + 64 * i, r);
  if (n_signers) n_signers[i] = count;
  if (!verdict) flag[i] = mgo_flag(cand, overlap);
}
KERNEL_SMALL void k_mgo_wave(MgParts in, size_t n, size_t bm_words, uint64_t wave_min, const uint8_t* verdict, uint8_t* flag, uint8_t* part_taken,
                             uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  __shared__ ClJacSlot part[BN_WAVE];
  __shared__ uint32_t cnt[BN_WAVE];
  const unsigned t = threadIdx.x;
  for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t len = verdict ? mgo_resum_len(in, i, true, flag, verdict) : mg_tuple_len(in, i, true);
    if (len < wave_min) continue;                        // wave_min >= 1: also every tuple the re-select masks out
    uint32_t* row = bits + i * bm_words;
    uint32_t cand, overlap;
    mgo_wave_select(cand, overlap, row, part_taken, bm_words, in, in.off[i], len, t);
    __syncthreads();
    mg_wave_partial(part[t].v, cnt[t], row, part_taken, bm_words, in, in.off[i], len, t);
    __syncthreads();
    for (unsigned stride = BN_WAVE / 2; stride >= 1; stride >>= 1) {
      if (t < stride) cl_tree_level(part, cnt, t, stride);
      __syncthreads();
    }
    if (t == 0) {
      cl_encode(agg + 64 * i, part[0].v);
      if (n_signers) n_signers[i] = cnt[0];
      if (!verdict) flag[i] = mgo_flag(cand, overlap);
    }
    __syncthreads();
  }
}
// behind the tuple check: the rows of the tuples that go the exact way are zeroed for the re-select, and the call's counters take what the
// check did (one ballot and one vector atomic per wave and counter, as k_clo_settle)
KERNEL_SMALL void k_mgo_settle(size_t n, size_t bm_words, ClScratch S, uint32_t* bits) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  const uint8_t flag = live ? S.flag[i] : (uint8_t)CLO_FINAL, verdict = live ? S.verdict[i] : (uint8_t)ST_OK;
  const bool checked = flag == CLO_CHECK, passed = checked && verdict == ST_OK, exact = clo_goes_exact(flag, verdict);
  if (exact)
    for (size_t w = 0; w < bm_words; ++w) bits[i * bm_words + w] = 0;
  const uint32_t n_checked = (uint32_t)__popcll(__ballot(checked)), n_passed = (uint32_t)__popcll(__ballot(passed)), n_exact = (uint32_t)__popcll(__ballot(exact));
  if (threadIdx.x == 0) {
    uint32_t* stats = S.stats + CLO_STAT_AT;
    if (n_checked) atomicAdd(&stats[0], n_checked);
    if (n_passed) atomicAdd(&stats[1], n_passed);
    if (n_exact) atomicAdd(&stats[2], n_exact);
  }
}
// slot j of a slice = partial base + j: queued for the exact verify iff it is a candidate of a tuple that goes the exact way.  The queue
// holds at most len entries (one per slot), and the workspace was reserved for a slice's length.
KERNEL_SMALL void k_mgo_queue(size_t len, uint64_t base, size_t n, const uint64_t* off, ClScratch S, const uint8_t* part_status, Ws ws) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j >= len) return;
  const size_t t = cl_tuple_of(base + j, S.end, off, n);
  if (clo_queued(part_status[base + j], t, n, S.flag, S.verdict)) ws.h_list[atomicAdd(&ws.h_cnt[0], 1u)] = (uint32_t)j;
}
// ... and the queue's length into the call's counters
KERNEL_SMALL void k_mgo_count(const uint32_t* h_cnt, uint32_t* stats) {
  if (threadIdx.x == 0 && h_cnt[0]) atomicAdd(&stats[CLO_STAT_AT + 3], h_cnt[0]);
}
// The route behind the hash, the range rule and the fills: pre-check, provisional select-and-sum, the tuple check in pieces of t_piece
// tuples, then the exact verify of the queued candidates in slices of p_piece partials and the re-select.  Everything is enqueued whether or
// not a tuple fails: the host never learns.  ms[0] = front end + provisional select-and-sum, ms[1] = aggregate keys of the union rows,
// ms[2] = the tuples' Miller loop and final exponentiation, ms[3] = fallback + re-select (a call in several pieces: the last piece's ms[1]
// boundary).
static int mg_optimistic(bn254_ctx* c, hipStream_t s, const MgParts& in, size_t n_parts, size_t n, size_t bm_words, uint32_t flags, size_t t_piece,
                         size_t p_piece, bool tables, const ClScratch& S, uint8_t* d_part_status, uint8_t* d_part_taken, uint8_t* d_agg_sigs,
                         uint32_t* d_signer_bits, uint32_t* d_n_signers) {
  int rc;
  const uint64_t wave_min = (uint64_t)c->merge_wave_min;
  const unsigned wave_grid = (unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS);
  const BmKeys K = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)c->n_keys};
  // 1. rules 1-3 of every partial; 2. the provisional select-and-sum of the candidates; 3. the tuples' flags
  k_mgo_precheck<<<grid_for(n_parts), BN_WAVE, 0, s>>>(n_parts, n, in.parts, in.rows, in.off, bm_words, flags, S, K, d_part_status);
  HIP_TRY(hipGetLastError());
  k_mgo_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, bm_words, wave_min, nullptr, S.flag, d_part_taken, d_signer_bits, d_agg_sigs, d_n_signers);
  HIP_TRY(hipGetLastError());
  k_mgo_wave<<<wave_grid, BN_WAVE, 0, s>>>(in, n, bm_words, wave_min, nullptr, S.flag, d_part_taken, d_signer_bits, d_agg_sigs, d_n_signers);
  HIP_TRY(hipGetLastError());
  PROF_MARK(1);
  // 4. the tuple check: the call's own outputs through the bitmap verify's kernels, decode flags 0 (an identity aggregate is legitimate)
  for (size_t lo = 0; lo < n; lo += t_piece) {
    const size_t len = n - lo < t_piece ? n - lo : t_piece;
    if ((rc = launch_decode_g1(c, s, d_agg_sigs + 64 * lo, len, 0, PL_P1X, BY_P1_INF, 0))) return rc;
    if ((rc = launch_clo_load_h(c, s, len, lo, S))) return rc;
    if ((rc = launch_bitmap_sum(c, s, d_signer_bits ? d_signer_bits + lo * bm_words : nullptr, bm_words, len, tables))) return rc;
    PROF_MARK(2);
    if ((rc = launch_verify_miller_fe(c, s, len, BN_PAIRS_VERIFY, 1, S.verdict + lo, false))) return rc;
  }
  PROF_MARK(3);
  k_mgo_settle<<<grid_for(n), BN_WAVE, 0, s>>>(n, bm_words, S, d_signer_bits);
  HIP_TRY(hipGetLastError());
  // 6. the candidates of the tuples that go the exact way, verified as the bitmap verify would over a queue; then those tuples selected again
  for (size_t lo = 0; lo < n_parts; lo += p_piece) {
    const size_t len = n_parts - lo < p_piece ? n_parts - lo : p_piece;
    if ((rc = launch_decode_g1(c, s, in.parts + 64 * lo, len, flags, PL_P1X, BY_P1_INF, 0))) return rc;
    if ((rc = launch_cl_spread(c, s, len, (uint64_t)lo, n, in.off, S))) return rc;
    HIP_TRY(hipMemsetAsync(c->ws.h_cnt, 0, sizeof(uint32_t), s));
    k_mgo_queue<<<grid_for(len), BN_WAVE, 0, s>>>(len, (uint64_t)lo, n, in.off, S, d_part_status, c->ws);
    HIP_TRY(hipGetLastError());
    k_mgo_count<<<1, BN_WAVE, 0, s>>>(c->ws.h_cnt, S.stats);
    HIP_TRY(hipGetLastError());
    if ((rc = launch_bitmap_sum_queued(c, s, in.rows ? in.rows + lo * bm_words : nullptr, bm_words, len, tables, c->ws.h_list, c->ws.h_cnt))) return rc;
    if ((rc = bn254_pair_miller_verify(len, c->ws, c->ws.h_list, c->ws.h_cnt, s))) return rc;
    if ((rc = bn254_pair_final_exp(len, c->ws, 1, d_part_status + lo, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  }
  k_mgo_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, bm_words, wave_min, S.verdict, S.flag, d_part_taken, d_signer_bits, d_agg_sigs, d_n_signers);
  HIP_TRY(hipGetLastError());
  k_mgo_wave<<<wave_grid, BN_WAVE, 0, s>>>(in, n, bm_words, wave_min, S.verdict, S.flag, d_part_taken, d_signer_bits, d_agg_sigs, d_n_signers);
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}

// both calls: !optimistic is the exact one
static int mg_merge_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_parts, const uint32_t* d_part_bits,
                           const uint64_t* d_part_off, size_t n_parts, size_t n, size_t bm_words, uint32_t flags, bool optimistic, uint8_t* d_part_status,
                           uint8_t* d_part_taken, uint8_t* d_tuple_status, uint8_t* d_agg_sigs, uint32_t* d_signer_bits, uint32_t* d_n_signers, void* stream) {
  MsgsLenScope msgs_len_scope(c);
  if (c) c->mgo_last_ran = 0;
  if (!c || bm_words > 0xFFFFFFFFu || n > 0xFFFFFFFFu || n_parts > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n && (!d_msgs || !d_msg_off || !d_part_off || !d_tuple_status || !d_agg_sigs || (bm_words && !d_signer_bits))) return BN254_E_BAD_ARGUMENT;
  if (n && n_parts && (!d_parts || !d_part_status || !d_part_taken || (bm_words && !d_part_bits))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_parts) || misaligned(d_part_bits) || misaligned(d_agg_sigs) || misaligned(d_signer_bits) || misaligned(d_n_signers) ||
      ((uintptr_t)d_msg_off & 7u) || ((uintptr_t)d_part_off & 7u))
    return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  // every buffer before the first kernel, as in the collect: the tuples are hashed, and the partials verified, in pieces of the slicing
  // rule's size; the scratch holds the whole call
  const size_t t_chunk = ws_chunk_for(c, n), p_chunk = n_parts ? ws_chunk_for(c, n_parts) : 0;
  const size_t t_piece = t_chunk ? t_chunk : n, p_piece = p_chunk ? p_chunk : n_parts;
  int rc = ws_reserve(c, t_piece > p_piece ? t_piece : p_piece);
  if (rc) return rc;
  ClScratch S;
  if ((rc = cl_scratch_reserve(c, n, &S))) return rc;
  c->clr_last_ran = c->clo_last_ran = 0;                 // the scratch is the collect's: its debug hooks have nothing of this call to read
  // the optimistic route: keys to sum, the lane-pair kernels the queue runs on, and enough partials.  Else the exact route, same bytes.
  const bool opt = optimistic && c->n_keys && c->key_lines && c->pair_lanes && n_parts && n_parts >= (size_t)c->merge_opt_min_parts;
  c->mgo_stats = S.stats + CLO_STAT_AT;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  const bool tables = bm_wants_tables(c);
  if ((rc = bm_prepare(c, s, tables))) return rc;        // the first call after a registration builds here, ahead of the timed intervals
  if (opt) HIP_TRY(hipMemsetAsync(S.stats, 0, CL_STAT_WORDS * sizeof(uint32_t), s));
  PROF_MARK(opt ? 0 : 1);
  // 1. hash once per tuple; 2. the range rule, the tuples' statuses, partial -> tuple
  if ((rc = cl_hash_and_plan(c, s, d_msgs, d_msg_off, d_part_off, n_parts, n, t_piece, S, d_tuple_status))) return rc;
  if (bm_words) HIP_TRY(hipMemsetAsync(d_signer_bits, 0, n * bm_words * sizeof(uint32_t), s));
  if (n_parts) {
    HIP_TRY(hipMemsetAsync(d_part_status, ST_INDEX_OOB, n_parts, s));
    HIP_TRY(hipMemsetAsync(d_part_taken, 0, n_parts, s));
  }
  if (opt) {
    const MgParts in = {d_parts, d_part_bits, d_part_off, d_part_status, d_tuple_status};
    if ((rc = mg_optimistic(c, s, in, n_parts, n, bm_words, flags, t_piece, p_piece, tables, S, d_part_status, d_part_taken, d_agg_sigs, d_signer_bits,
                            d_n_signers)))
      return rc;
    c->mgo_last_ran = 1;                                 // only a call that enqueued everything has something for the debug hook to read
    return 0;
  }
  // 3. the bitmap verify of the partials
  for (size_t lo = 0; lo < n_parts; lo += p_piece) {
    const size_t len = n_parts - lo < p_piece ? n_parts - lo : p_piece;
    if ((rc = mg_verify_slice(c, s, d_parts, d_part_bits, d_part_off, n, lo, len, bm_words, flags, tables, S, d_part_status))) return rc;
  }
  if (!n_parts) { PROF_MARK(2); PROF_MARK(3); PROF_MARK(4); }
  // 4. select-and-sum, once, behind the last slice
  const MgParts in = {d_parts, d_part_bits, d_part_off, d_part_status, d_tuple_status};
  const uint64_t wave_min = (uint64_t)c->merge_wave_min;
  k_mg_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, bm_words, wave_min, d_part_taken, d_signer_bits, d_agg_sigs, d_n_signers);
  HIP_TRY(hipGetLastError());
  k_mg_wave<<<(unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS), BN_WAVE, 0, s>>>(in, n, bm_words, wave_min, d_part_taken, d_signer_bits, d_agg_sigs,
                                                                                           d_n_signers);
  PROF_MARK(0);
  prof_done(c, EV_COLLECT);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the host-pointer form of both
static int mg_merge_host(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* parts, const uint32_t* part_bits,
                         const uint64_t* part_off, size_t n_parts, size_t n, size_t bm_words, uint32_t flags, bool optimistic, uint8_t* part_status,
                         uint8_t* part_taken, uint8_t* tuple_status, uint8_t* agg_sigs, uint32_t* signer_bits, uint32_t* n_signers) {
  MsgsLenScope msgs_len_scope(c);
  if (c) c->mgo_last_ran = 0;
  if (!c || bm_words > 0xFFFFFFFFu || n > 0xFFFFFFFFu || n_parts > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n && (!msg_off || !part_off || !tuple_status || !agg_sigs || (bm_words && !signer_bits))) return BN254_E_BAD_ARGUMENT;
  if (n && n_parts && (!parts || !part_status || !part_taken || (bm_words && !part_bits))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, msg_off, n)) return BN254_E_BAD_ARGUMENT;
  if (part_off[0] != 0 || !offsets_ok(part_off, n) || part_off[n] != n_parts) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)msg_off[n]), *d_msg_off = st.in(1, msg_off, (n + 1) * sizeof(uint64_t));
  const uint8_t *d_parts = st.in(2, parts, n_parts * 64), *d_bits = st.in(3, part_bits, n_parts * bm_words * sizeof(uint32_t));
  const uint8_t* d_part_off = st.in(4, part_off, (n + 1) * sizeof(uint64_t));
  // the six outputs share one slot: the aligned ones first
  const size_t o_bits = n * 64, o_cnt = o_bits + n * bm_words * sizeof(uint32_t), o_pst = o_cnt + n * sizeof(uint32_t), o_tkn = o_pst + n_parts,
               o_tst = o_tkn + n_parts;
  uint8_t* d_out = st.out(5, o_tst + n);
  if (st.ok()) {
    st.copy_back(agg_sigs, d_out, n * 64);
    st.copy_back(signer_bits, d_out + o_bits, n * bm_words * sizeof(uint32_t));
    st.copy_back(n_signers, d_out + o_cnt, n * sizeof(uint32_t));
    st.copy_back(part_status, d_out + o_pst, n_parts);
    st.copy_back(part_taken, d_out + o_tkn, n_parts);
    st.copy_back(tuple_status, d_out + o_tst, n);
  }
  if (st.ok())
    st.rc = mg_merge_device(c, d_msgs, (const uint64_t*)d_msg_off, d_parts, bm_words ? (const uint32_t*)d_bits : nullptr, (const uint64_t*)d_part_off, n_parts, n,
                            bm_words, flags, optimistic, d_out + o_pst, d_out + o_tkn, d_out + o_tst, d_out, (uint32_t*)(d_out + o_bits),
                            n_signers ? (uint32_t*)(d_out + o_cnt) : nullptr, nullptr);
  return st.finish();
}

extern "C" {

int bn254_batch_merge_keyed_bitmap_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_parts,
                                          const uint32_t* d_part_bits, const uint64_t* d_part_off, size_t n_parts, size_t n, size_t bm_words,
                                          uint32_t flags, uint8_t* d_part_status, uint8_t* d_part_taken, uint8_t* d_tuple_status, uint8_t* d_agg_sigs,
                                          uint32_t* d_signer_bits, uint32_t* d_n_signers, void* stream) {
  return mg_merge_device(c, d_msgs, d_msg_off, d_parts, d_part_bits, d_part_off, n_parts, n, bm_words, flags, false, d_part_status, d_part_taken, d_tuple_status,
                         d_agg_sigs, d_signer_bits, d_n_signers, stream);
}
int bn254_batch_merge_keyed_bitmap(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* parts, const uint32_t* part_bits,
                                   const uint64_t* part_off, size_t n_parts, size_t n, size_t bm_words, uint32_t flags, uint8_t* part_status,
                                   uint8_t* part_taken, uint8_t* tuple_status, uint8_t* agg_sigs, uint32_t* signer_bits, uint32_t* n_signers) {
  return mg_merge_host(c, msgs, msg_off, parts, part_bits, part_off, n_parts, n, bm_words, flags, false, part_status, part_taken, tuple_status, agg_sigs,
                       signer_bits, n_signers);
}
int bn254_batch_merge_keyed_bitmap_optimistic_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_parts,
                                                     const uint32_t* d_part_bits, const uint64_t* d_part_off, size_t n_parts, size_t n, size_t bm_words,
                                                     uint32_t flags, uint8_t* d_part_status, uint8_t* d_part_taken, uint8_t* d_tuple_status,
                                                     uint8_t* d_agg_sigs, uint32_t* d_signer_bits, uint32_t* d_n_signers, void* stream) {
  return mg_merge_device(c, d_msgs, d_msg_off, d_parts, d_part_bits, d_part_off, n_parts, n, bm_words, flags, true, d_part_status, d_part_taken, d_tuple_status,
                         d_agg_sigs, d_signer_bits, d_n_signers, stream);
}
int bn254_batch_merge_keyed_bitmap_optimistic(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* parts, const uint32_t* part_bits,
                                              const uint64_t* part_off, size_t n_parts, size_t n, size_t bm_words, uint32_t flags, uint8_t* part_status,
                                              uint8_t* part_taken, uint8_t* tuple_status, uint8_t* agg_sigs, uint32_t* signer_bits, uint32_t* n_signers) {
  return mg_merge_host(c, msgs, msg_off, parts, part_bits, part_off, n_parts, n, bm_words, flags, true, part_status, part_taken, tuple_status, agg_sigs,
                       signer_bits, n_signers);
}

}  // extern "C"
