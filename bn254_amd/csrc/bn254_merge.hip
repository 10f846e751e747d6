// Translation unit of libbn254hip.so: merging partial signer-bitmap aggregates into one aggregate per message (include/bn254_hip.h:
// bn254_batch_merge_keyed_bitmap[_device]) — the inner node of an aggregation tree.  The front end is the collect's
// (bn254_collect.hip: hash once per tuple, range rule, spread of H(m) over the tuple's partials), the verify of a slice of partials is the
// bitmap verify's (bn254_bitmap.hip: bm_prepare, launch_bitmap_sum; launch_verify_miller_fe), and the first-fit select-and-sum in two
// layouts is this unit's; its walk and arithmetic are bn254_merge.h, shared with the CPU suite's host compilation.  The arguments travel as
// the collect's record (bn254_host.h: ClCall — items = the partials, aux = their rows), through the collect's checks and staging.
// bn254_batch_merge_keyed_bitmap_optimistic[_device] verifies each tuple's provisional SUM once, by the same kernels, and
// sends only the candidates of the tuples that fail — or hold an overlap — through a device-side queue into the bitmap verify's lane-pair
// kernels (mg_optimistic; the tuple check, its settle and the queue are the optimistic collect's: clo_tuple_check, clo_queue_slice).
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
static int mg_verify_slice(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t lo, size_t len, bool tables, const ClScratch& S) {
  int rc;
  if ((rc = cl_slice_head(c, s, a, lo, len, S))) return rc;
  if ((rc = launch_bitmap_sum(c, s, a.aux ? a.aux + lo * a.bm_words : nullptr, a.bm_words, len, tables))) return rc;
  PROF_MARK(2);
  if ((rc = launch_verify_miller_fe(c, s, len, BN_PAIRS_VERIFY, 1, a.item_status + lo, true))) return rc;
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
// rows zeroed by k_clo_settle) over the final statuses — a tuple that does not go the exact way has length 0 and nothing of it is written.
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
// The route behind the hash, the range rule and the fills: pre-check, provisional select-and-sum, the tuple check in pieces of t_piece
// tuples, then the exact verify of the queued candidates in slices of p_piece partials and the re-select.  Everything is enqueued whether or
// not a tuple fails: the host never learns.  ms[0] = front end + provisional select-and-sum, ms[1] = aggregate keys of the union rows,
// ms[2] = the tuples' Miller loop and final exponentiation, ms[3] = fallback + re-select (a call in several pieces: the last piece's ms[1]
// boundary).
static int mg_optimistic(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t t_piece, size_t p_piece, bool tables, const ClScratch& S) {
  int rc;
  const size_t n = a.n, n_parts = a.n_items;
  const MgParts in = {a.items, a.aux, a.off, a.item_status, a.tuple_status};
  const uint64_t wave_min = (uint64_t)c->merge_wave_min;
  const unsigned wave_grid = (unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS);
  const BmKeys K = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)c->n_keys};
  // 1. rules 1-3 of every partial; 2. the provisional select-and-sum of the candidates; 3. the tuples' flags
  k_mgo_precheck<<<grid_for(n_parts), BN_WAVE, 0, s>>>(n_parts, n, in.parts, in.rows, in.off, a.bm_words, a.flags, S, K, a.item_status);
  HIP_TRY(hipGetLastError());
  k_mgo_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, nullptr, S.flag, a.item_taken, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  k_mgo_wave<<<wave_grid, BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, nullptr, S.flag, a.item_taken, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  PROF_MARK(1);
  // 4. the tuple check of the call's own outputs, and 5. what it settles: the collect's (bn254_collect.hip: clo_tuple_check)
  if ((rc = clo_tuple_check(c, s, a, t_piece, S))) return rc;
  // 6. the candidates of the tuples that go the exact way, verified as the bitmap verify would over a queue; then those tuples selected again
  for (size_t lo = 0; lo < n_parts; lo += p_piece) {
    const size_t len = n_parts - lo < p_piece ? n_parts - lo : p_piece;
    if ((rc = clo_queue_slice(c, s, a, lo, len, S))) return rc;
    if ((rc = launch_bitmap_sum_queued(c, s, in.rows ? in.rows + lo * a.bm_words : nullptr, a.bm_words, len, tables, c->ws.h_list, c->ws.h_cnt))) return rc;
    if ((rc = bn254_pair_miller_verify(len, c->ws, c->ws.h_list, c->ws.h_cnt, s))) return rc;
    if ((rc = bn254_pair_final_exp(len, c->ws, 1, a.item_status + lo, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  }
  k_mgo_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, S.verdict, S.flag, a.item_taken, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  k_mgo_wave<<<wave_grid, BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, S.verdict, S.flag, a.item_taken, a.signer_bits, a.agg_sigs, a.n_signers);
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the merge's own check (ahead of the common ones): the partials' taken flags and, when a row has words, their rows
static bool mg_parts_ok(const ClCall& a) { return !(a.n && a.n_items && (!a.item_taken || (a.bm_words && !a.aux))); }
// both calls: !optimistic is the exact one
static int mg_merge_device(bn254_ctx* c, const ClCall& a, bool optimistic, void* stream) {
  if (g1c_flag(a.flags))                                // compressed partials: staged once, in front of the hash and of any slicing
    return cl_g1c_call(c, a, stream, [&](const ClCall& d) { return mg_merge_device(c, d, optimistic, stream); });
  MsgsLenScope msgs_len_scope(c);
  if (c) c->mgo_last_ran = 0;
  int rc = BN254_E_BAD_ARGUMENT;
  if (!mg_parts_ok(a) || !cl_checks_device(c, a, &rc)) return rc;
  const size_t n = a.n, n_parts = a.n_items;
  // every buffer before the first kernel, as in the collect: the tuples are hashed, and the partials verified, in pieces of the slicing
  // rule's size; the scratch holds the whole call
  const size_t t_chunk = ws_chunk_for(c, n), p_chunk = n_parts ? ws_chunk_for(c, n_parts) : 0;
  const size_t t_piece = t_chunk ? t_chunk : n, p_piece = p_chunk ? p_chunk : n_parts;
  if ((rc = ws_reserve(c, t_piece > p_piece ? t_piece : p_piece))) return rc;
  ClScratch S;
  if ((rc = cl_scratch_reserve(c, n, &S))) return rc;
  c->clr_last_ran = c->clo_last_ran = c->tho_last_ran = 0;                 // the scratch is the collect's: its debug hooks have nothing of this call to read
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
  if ((rc = cl_hash_and_plan(c, s, a, t_piece, S))) return rc;
  if (a.bm_words) HIP_TRY(hipMemsetAsync(a.signer_bits, 0, n * a.bm_words * sizeof(uint32_t), s));
  if (n_parts) {
    HIP_TRY(hipMemsetAsync(a.item_status, ST_INDEX_OOB, n_parts, s));
    HIP_TRY(hipMemsetAsync(a.item_taken, 0, n_parts, s));
  }
  if (opt) {
    if ((rc = mg_optimistic(c, s, a, t_piece, p_piece, tables, S))) return rc;
    c->mgo_last_ran = 1;                                 // only a call that enqueued everything has something for the debug hook to read
    return 0;
  }
  // 3. the bitmap verify of the partials
  for (size_t lo = 0; lo < n_parts; lo += p_piece) {
    const size_t len = n_parts - lo < p_piece ? n_parts - lo : p_piece;
    if ((rc = mg_verify_slice(c, s, a, lo, len, tables, S))) return rc;
  }
  if (!n_parts) { PROF_MARK(2); PROF_MARK(3); PROF_MARK(4); }
  // 4. select-and-sum, once, behind the last slice
  const MgParts in = {a.items, a.aux, a.off, a.item_status, a.tuple_status};
  const uint64_t wave_min = (uint64_t)c->merge_wave_min;
  k_mg_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, a.item_taken, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  k_mg_wave<<<(unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, a.item_taken, a.signer_bits, a.agg_sigs,
                                                                                           a.n_signers);
  PROF_MARK(0);
  prof_done(c, EV_COLLECT);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the host-pointer form of both
static int mg_merge_host(bn254_ctx* c, const ClCall& a, bool optimistic) {
  MsgsLenScope msgs_len_scope(c);
  if (c) c->mgo_last_ran = 0;
  int rc = BN254_E_BAD_ARGUMENT;
  if (!mg_parts_ok(a) || !cl_checks_host(c, a, &rc)) return rc;
  HostStaging st(c);
  ClCall d;
  cl_stage(st, a, a.bm_words, 5, &d);
  if (st.ok()) st.rc = mg_merge_device(c, d, optimistic, nullptr);
  return st.finish();
}

extern "C" {

int bn254_batch_merge_keyed_bitmap_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_parts,
                                          const uint32_t* d_part_bits, const uint64_t* d_part_off, size_t n_parts, size_t n, size_t bm_words,
                                          uint32_t flags, uint8_t* d_part_status, uint8_t* d_part_taken, uint8_t* d_tuple_status, uint8_t* d_agg_sigs,
                                          uint32_t* d_signer_bits, uint32_t* d_n_signers, void* stream) {
  const ClCall a = {.msgs = d_msgs, .msg_off = d_msg_off, .items = d_parts, .aux = d_part_bits, .off = d_part_off, .n_items = n_parts, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = d_part_status, .item_taken = d_part_taken, .tuple_status = d_tuple_status,
                    .agg_sigs = d_agg_sigs, .signer_bits = d_signer_bits, .n_signers = d_n_signers};
  return mg_merge_device(c, a, false, stream);
}
int bn254_batch_merge_keyed_bitmap(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* parts, const uint32_t* part_bits,
                                   const uint64_t* part_off, size_t n_parts, size_t n, size_t bm_words, uint32_t flags, uint8_t* part_status,
                                   uint8_t* part_taken, uint8_t* tuple_status, uint8_t* agg_sigs, uint32_t* signer_bits, uint32_t* n_signers) {
  const ClCall a = {.msgs = msgs, .msg_off = msg_off, .items = parts, .aux = part_bits, .off = part_off, .n_items = n_parts, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = part_status, .item_taken = part_taken, .tuple_status = tuple_status,
                    .agg_sigs = agg_sigs, .signer_bits = signer_bits, .n_signers = n_signers};
  return mg_merge_host(c, a, false);
}
int bn254_batch_merge_keyed_bitmap_optimistic_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_parts,
                                                     const uint32_t* d_part_bits, const uint64_t* d_part_off, size_t n_parts, size_t n, size_t bm_words,
                                                     uint32_t flags, uint8_t* d_part_status, uint8_t* d_part_taken, uint8_t* d_tuple_status,
                                                     uint8_t* d_agg_sigs, uint32_t* d_signer_bits, uint32_t* d_n_signers, void* stream) {
  const ClCall a = {.msgs = d_msgs, .msg_off = d_msg_off, .items = d_parts, .aux = d_part_bits, .off = d_part_off, .n_items = n_parts, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = d_part_status, .item_taken = d_part_taken, .tuple_status = d_tuple_status,
                    .agg_sigs = d_agg_sigs, .signer_bits = d_signer_bits, .n_signers = d_n_signers};
  return mg_merge_device(c, a, true, stream);
}
int bn254_batch_merge_keyed_bitmap_optimistic(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* parts, const uint32_t* part_bits,
                                              const uint64_t* part_off, size_t n_parts, size_t n, size_t bm_words, uint32_t flags, uint8_t* part_status,
                                              uint8_t* part_taken, uint8_t* tuple_status, uint8_t* agg_sigs, uint32_t* signer_bits, uint32_t* n_signers) {
  const ClCall a = {.msgs = msgs, .msg_off = msg_off, .items = parts, .aux = part_bits, .off = part_off, .n_items = n_parts, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = part_status, .item_taken = part_taken, .tuple_status = tuple_status,
                    .agg_sigs = agg_sigs, .signer_bits = signer_bits, .n_signers = n_signers};
  return mg_merge_host(c, a, true);
}

}  // extern "C"
