// Translation unit of libbn254hip.so: building signer-bitmap aggregates from the signers' individual signatures (include/bn254_hip.h:
// bn254_batch_collect_keyed_bitmap[_device]) — the producer half of the bitmap verify.  Hash once per tuple, spread H(m)
// over the tuple's share slots, the keyed verify of the slots unchanged, then select-and-sum in two layouts.  The bookkeeping and the
// arithmetic of the kernels are bn254_collect.h, shared with the CPU suite's host compilation.
// bn254_batch_collect_keyed_bitmap_randomized[_device] is the same call with the slots verified by the grouped checks of the
// randomised keyed verify (bn254_rand.hip: launch_keyed_rand_checks): the shares of a slice grouped by key across its tuples.
// bn254_batch_collect_keyed_bitmap_optimistic[_device] verifies each tuple's SUM once, by the bitmap verify's kernels
// (bn254_bitmap.hip: bm_prepare, launch_bitmap_sum; launch_verify_miller_fe), and sends only the candidates of the tuples that fail — or
// have a duplicate, or too few candidates — through a device-side queue into the exact keyed kernels (cl_optimistic).
// The unit also holds what the whole family shares (bn254_host.h): every extern "C" function fills one record of its arguments (ClCall), and
// the checks, the staging of a host form, the front end, the head of a slice and the optimistic route's tuple check and queue take that
// record — for the merge of partial aggregates (bn254_merge.hip) and the threshold call (bn254_threshold.hip: cl_collect_run) as for the collect.
// Per-share semantics: ECDSA::verify (/root/reference/src/ecdsa.rs:49-64); the sum: `Add for Signature` (src/types.rs:264-270).
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

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"
#include "bn254_aggd_plan.h"

// per tuple, outside the (sliced) workspace: the scans of the range rule, H(m) with its identity flag and hash status
#define CL_HASH_WORDS (2 * BN_LIMBS)
// ... and, in front, what the randomised slices of the call did: {slices, groups checked, groups failed, shares re-checked exactly}, then what
// the optimistic route did: {tuples checked, tuples passed, tuples sent the exact way, shares verified exactly} (bn254_host.h: CL_STAT_WORDS,
// CLO_STAT_AT); behind, that route's flag (bn254_collect.h: CLO_*) and tuple-check verdict per tuple
// (struct ClScratch: bn254_host.h — the merge of partial aggregates, bn254_merge.hip, shares the scratch and the front end)
static ClScratch cl_scratch(Carve& c, size_t n) {
  ClScratch b;
  b.stats = c.take<uint32_t>(CL_STAT_WORDS);
  b.mx = c.take<uint64_t>(n), b.hi = c.take<uint64_t>(n), b.end = c.take<uint64_t>(n);
  b.tot = c.take<uint64_t>((n + AGGD_SCAN_WG - 1) / AGGD_SCAN_WG);
  b.hpt = c.take<int32_t>(n * CL_HASH_WORDS);
  b.hinf = c.take<uint8_t>(n), b.hst = c.take<uint8_t>(n);
  b.flag = c.take<uint8_t>(n), b.verdict = c.take<uint8_t>(n);
  return b;
}

// H(m) of the tuples base .. base + len, hashed into workspace entries 0 .. len, into the call's scratch
KERNEL_SMALL void k_cl_save(size_t len, size_t base, Ws ws, ClScratch S) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= len) return;
  const Fp x = ws_load_fp(ws, PL_P2X, i), y = ws_load_fp(ws, PL_P2Y, i);
  int32_t* w = S.hpt + (base + i) * CL_HASH_WORDS;
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) { w[k] = x.v[k]; w[BN_LIMBS + k] = y.v[k]; }
  S.hinf[base + i] = ws_byte(ws, BY_P2_INF, i);
  S.hst[base + i] = ws_byte(ws, BY_ST_HASH, i);
}
// the range rule and the tuple's status: 2 for a refused range (it gets no shares), else the hash status of its message
KERNEL_SMALL void k_cl_plan(size_t n, uint64_t n_shares, const uint64_t* off, ClScratch S, uint8_t* tuple_status) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const bool ok = cl_range_ok(off[i], off[i + 1], n_shares, i == 0, i ? S.mx[i - 1] : 0);
  S.hi[i] = ok ? off[i + 1] : 0;
  tuple_status[i] = ok ? S.hst[i] : (uint8_t)ST_INDEX_OOB;
}
// slot j of a slice = share base + j: its tuple's H(m) and hash status, as launch_hash_rounds would have left them for the message repeated.
// A share of no accepted tuple reads IndexOutOfBounds whatever its bytes, and walks on with the generator.
KERNEL_SMALL void k_cl_spread(size_t len, uint64_t base, size_t n, const uint64_t* off, ClScratch S, Ws ws) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j >= len) return;
  const size_t t = cl_tuple_of(base + j, S.end, off, n);
  if (t >= n) {
    G1Affine g;
    g1_set_generator(g);
    ws_store_g1(ws, PL_P2X, BY_P2_INF, j, g);
    ws_byte(ws, BY_ST_HASH, j) = ST_OK;
    ws_byte(ws, BY_ST_DECODE, j) = ST_INDEX_OOB;
    return;
  }
  const int32_t* w = S.hpt + t * CL_HASH_WORDS;
  Fp x, y;
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) { x.v[k] = w[k]; y.v[k] = w[BN_LIMBS + k]; }
  ws_store_fp(ws, PL_P2X, j, x);
  ws_store_fp(ws, PL_P2Y, j, y);
  ws_byte(ws, BY_P2_INF, j) = S.hinf[t];
  ws_byte(ws, BY_ST_HASH, j) = S.hst[t];
}

// ---- what bn254_merge.hip and bn254_threshold.hip share with this unit (bn254_host.h): the checks and the staging of a call, the scratch,
// steps 1 and 2 of every call, and the head of a slice ------------------------------------------------------------------------------------------
static int cl_checks_head(const bn254_ctx* c, const ClCall& a, bool device) {
  if (!c || a.bm_words > 0xFFFFFFFFu || a.n > 0xFFFFFFFFu || a.n_items > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (a.n && ((device && !a.msgs) || !a.msg_off || !a.off || !a.tuple_status || !a.agg_sigs || (a.bm_words && !a.signer_bits))) return BN254_E_BAD_ARGUMENT;
  if (a.n && a.n_items && (!a.items || !a.item_status)) return BN254_E_BAD_ARGUMENT;
  return 0;
}
bool cl_checks_host(bn254_ctx* c, const ClCall& a, int* rc) {
  if ((*rc = cl_checks_head(c, a, false)) || a.n == 0) return false;
  if (const hipError_t e = hipSetDevice(c->device)) *rc = -(int)e;
  else if (!msgs_ok(a.msgs, a.msg_off, a.n) || a.off[0] != 0 || !offsets_ok(a.off, a.n) || a.off[a.n] != a.n_items) *rc = BN254_E_BAD_ARGUMENT;
  return *rc == 0;
}
bool cl_checks_device(bn254_ctx* c, const ClCall& a, int* rc) {
  if ((*rc = cl_checks_head(c, a, true)) || a.n == 0) return false;
  if (misaligned(a.items) || misaligned(a.aux) || misaligned(a.agg_sigs) || misaligned(a.signer_bits) || misaligned(a.n_signers) ||
      ((uintptr_t)a.msg_off & 7u) || ((uintptr_t)a.off & 7u))
    *rc = BN254_E_MISALIGNED;
  else if (const hipError_t e = hipSetDevice(c->device)) *rc = -(int)e;
  return *rc == 0;
}
void cl_stage(HostStaging& st, const ClCall& a, size_t aux_words, int out_slot, ClCall* d) {
  const size_t n = a.n, m = a.n_items, row = a.bm_words * sizeof(uint32_t), taken = a.item_taken ? m : 0;
  *d = a;
  d->msgs = st.in(0, a.msgs, (size_t)a.msg_off[n]);
  d->msg_off = (const uint64_t*)st.in(1, a.msg_off, (n + 1) * sizeof(uint64_t));
  d->items = st.in(2, a.items, m * g1_item_bytes(a.flags));
  const uint8_t* d_aux = st.in(3, a.aux, m * aux_words * sizeof(uint32_t));
  d->aux = aux_words ? (const uint32_t*)d_aux : nullptr;
  d->off = (const uint64_t*)st.in(4, a.off, (n + 1) * sizeof(uint64_t));
  // the outputs share one slot: the aligned ones first
  const size_t o_bits = n * 64, o_cnt = o_bits + n * row, o_ist = o_cnt + n * sizeof(uint32_t), o_tkn = o_ist + m, o_tst = o_tkn + taken;
  uint8_t* d_out = st.out(out_slot, o_tst + n);
  if (!st.ok()) return;
  d->agg_sigs = d_out, d->signer_bits = (uint32_t*)(d_out + o_bits), d->n_signers = a.n_signers ? (uint32_t*)(d_out + o_cnt) : nullptr;
  d->item_status = d_out + o_ist, d->item_taken = a.item_taken ? d_out + o_tkn : nullptr, d->tuple_status = d_out + o_tst;
  st.copy_back(a.agg_sigs, d->agg_sigs, n * 64);
  st.copy_back(a.signer_bits, d->signer_bits, n * row);
  st.copy_back(a.n_signers, d_out + o_cnt, n * sizeof(uint32_t));
  st.copy_back(a.item_status, d->item_status, m);
  st.copy_back(a.item_taken, d->item_taken, taken);
  st.copy_back(a.tuple_status, d->tuple_status, n);
}
int cl_scratch_reserve(bn254_ctx* c, size_t n, ClScratch* S) {
  Carve size(nullptr);
  cl_scratch(size, n);
  if (const int rc = scratch_reserve(c, &c->collect_buf, &c->collect_cap, size.used)) return rc;
  Carve carve(c->collect_buf);
  *S = cl_scratch(carve, n);
  return 0;
}
// 1. hash once per tuple, in pieces of t_piece tuples; 2. the range rule over a.off against n_items, the tuples' statuses, item -> tuple
int cl_hash_and_plan(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t t_piece, const ClScratch& S) {
  int rc;
  for (size_t lo = 0; lo < a.n; lo += t_piece) {
    const size_t len = a.n - lo < t_piece ? a.n - lo : t_piece;
    if ((rc = launch_hash_rounds(c, s, a.msgs, a.msg_off + lo, len, PL_P2X, BY_P2_INF, nullptr))) return rc;
    k_cl_save<<<grid_for(len), BN_WAVE, 0, s>>>(len, lo, c->ws, S);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = bn254_aggd_scan_max(s, a.off, a.n, S.mx, S.tot))) return rc;
  k_cl_plan<<<grid_for(a.n), BN_WAVE, 0, s>>>(a.n, (uint64_t)a.n_items, a.off, S, a.tuple_status);
  HIP_TRY(hipGetLastError());
  return bn254_aggd_scan_max(s, S.hi, a.n, S.end, S.tot);
}
// Profiling: every slice records its intervals, so the last one's stay (a slice behind the first opens its own front end; the first one's
// began with the hash)
int cl_slice_head(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t lo, size_t len, const ClScratch& S) {
  if (lo) PROF_MARK(1);
  if (const int rc = launch_decode_g1(c, s, a.items + 64 * lo, len, a.flags, PL_P1X, BY_P1_INF, 0)) return rc;
  k_cl_spread<<<grid_for(len), BN_WAVE, 0, s>>>(len, (uint64_t)lo, a.n, a.off, S, c->ws);
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- select-and-sum (both kernels run on the zeroed output rows; a tuple is taken by exactly one of them, by its own length) ---------------
// lane per tuple, the tuples below wave_min shares.  No early return: the additions vote across the wave (see k_bm_sum); a lane whose
// tuple is long, or past the end, walks identities.
KERNEL_SMALL void k_cl_sum_lane(ClShares in, size_t n, size_t bm_words, uint64_t wave_min, uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  uint64_t len = cl_tuple_len(in, live ? i : 0, live);
  const bool mine = live && len < wave_min;
  if (!mine) len = 0;
  G1Jac acc;
  uint32_t count;
  cl_lane_sum(acc, count, bits + (mine ? i : 0) * bm_words, bm_words, in, mine ? in.off[i] : 0, len);
  G1Affine r;
  jac_to_affine(r, acc);
  if (!mine) return;
  encode_g1(agg + 64 * i, r);
  if (n_signers) n_signers[i] = count;
}
// wave per tuple, the others: a wave leaves a short tuple at once (wave-uniformly); tuples beyond the grid by stride.  The partial sums are
// accumulated in place in LDS, through generic references (as k_rand_scale keeps its accumulator): every limb is a flat access.  Measured,
// the kernel sums one tuple of 4 096 shares in 0.27 ms beside a 2.2 ms verify, so the partial sums were not moved into registers.
KERNEL_SMALL void k_cl_sum_wave(ClShares in, size_t n, size_t bm_words, uint64_t wave_min, uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  __shared__ ClJacSlot part[BN_WAVE];
  __shared__ uint32_t cnt[BN_WAVE];
  const unsigned t = threadIdx.x;
  for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t len = cl_tuple_len(in, i, true);
    if (len < wave_min) continue;
    cl_wave_partial(part[t].v, cnt[t], bits + i * bm_words, bm_words, in, in.off[i], len, t);
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

// one slice of the shares: decode, spread, the keyed verify of the slots; statuses at the shares' own positions
static int cl_verify_slice(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t lo, size_t len, const ClScratch& S) {
  int rc;
  if ((rc = cl_slice_head(c, s, a, lo, len, S))) return rc;
  PROF_MARK(2);
  if (c->n_keys == 0 || !c->key_lines) {               // nothing registered: every share that decodes is out of range
    if ((rc = launch_keyed_no_keys(c, s, len, a.item_status + lo))) return rc;
    PROF_MARK(3);
  } else if ((rc = launch_keyed_miller_fe(c, s, len, a.aux + lo, a.item_status + lo, ctx_key_table(c), c->key_xy))) return rc;
  PROF_MARK(4);
  return 0;
}

// ---- the randomised route -------------------------------------------------------------------------------------------------------------------
// what a slice's grouped checks did, added to the call's counters: one wave behind launch_keyed_rand_checks, which left {groups, slots} in
// meta, the groups' verdicts in group_st and the length of the exact re-check's queue in h_cnt[0]
KERNEL_SMALL void k_cl_rand_count(const uint32_t* meta, const uint8_t* group_st, const uint32_t* h_cnt, uint32_t* stats) {
  const unsigned t = threadIdx.x;
  uint32_t failed = 0;
  for (uint32_t g = t; g < meta[0]; g += BN_WAVE) failed += group_st[g] != ST_OK ? 1u : 0u;
  if (failed) atomicAdd(&stats[2], failed);
  if (t == 0) { atomicAdd(&stats[0], 1u); atomicAdd(&stats[1], meta[0]); atomicAdd(&stats[3], h_cnt[0]); }
}
// The shares per slice of the randomised route.  A slice of len shares needs keyed_rand_need(c, len).ws_entries workspace entries — the
// slots and, behind them, one entry per group — so the length is chosen for the ENTRIES that fit, never reserved as len alone:
//   * BN254_OPT_MAX_CHUNK set: that many shares, as the caller asked, and the entries that go with them;
//   * else everything in one slice when the entries of the whole call fit (ws_chunk_for prices entries, whatever they hold);
//   * else the largest multiple of 256 shares whose entries fit in what ws_chunk_for allows: len + len / 64 + n_keys + 1 <= entries.
// 0 = the allowance holds no slice with its groups: the caller takes the exact route (same bytes).
static size_t cl_rand_slice_len(bn254_ctx* c, size_t n_shares) {
  if (c->max_chunk > 0) return n_shares < (size_t)c->max_chunk ? n_shares : (size_t)c->max_chunk;
  const size_t entries = ws_chunk_for(c, keyed_rand_need(c, n_shares).ws_entries);
  if (entries == 0) return n_shares;
  const size_t fixed = c->n_keys + 1 + 256;
  if (entries <= fixed + 256) return 0;
  const size_t len = ((entries - fixed) / 65 * 64) & ~(size_t)255;
  return len < n_shares ? len : n_shares;
}
// ... and a slice whose padded runs (64 slots per group) would not be numbered in 32 bits is not grouped at all
static bool cl_rand_slots_fit(const bn254_ctx* c, size_t len) { return keyed_rand_need(c, len).groups_max <= (size_t)0x03FFFFFF; }
// one slice of the shares on that route: decode and spread as cl_verify_slice, then the grouped checks of the slots with the weights of the
// shares' own indices (index_base = lo).  The spread has put H(m) and the hash status of its tuple into every slot, which is the layout
// k_krand_prepare and the exact re-check read.  ms[2] = grouping + scalar ladders, ms[3] = group checks + exact re-checks.
static int cl_verify_slice_rand(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t lo, size_t len, const RandSeed& seed, int mode, const ClScratch& S) {
  int rc;
  if ((rc = cl_slice_head(c, s, a, lo, len, S))) return rc;
  PROF_MARK(2);
  if ((rc = launch_keyed_rand_checks(c, s, len, a.aux + lo, seed, mode, (uint64_t)lo, a.item_status + lo))) return rc;
  k_cl_rand_count<<<1, BN_WAVE, 0, s>>>(keyed_rand_meta(c), keyed_rand_group_st(c), c->ws.h_cnt, S.stats);
  HIP_TRY(hipGetLastError());
  PROF_MARK(4);
  return 0;
}

// ---- the optimistic route (the steps are bn254_collect.h's clo_*) ------------------------------------------------------------
// rules 1-3 of every share of an accepted tuple, straight from the caller's bytes: no workspace, no pairing.  A share of nobody keeps the 2
// the status array was filled with.
KERNEL_SMALL void k_clo_precheck(size_t n_shares, size_t n, const uint8_t* shares, const uint32_t* key, const uint64_t* off, uint32_t flags, ClScratch S,
                                 const uint8_t* key_st, uint32_t n_keys, uint8_t* share_status) {
  const size_t s = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (s >= n_shares) return;
  const size_t t = cl_tuple_of(s, S.end, off, n);
  if (t >= n) return;
  share_status[s] = clo_precheck(shares + 64 * s, flags, key[s], key_st, n_keys, S.hst[t]);
}
// the select-and-sum of k_cl_sum_lane / k_cl_sum_wave with refused claims reported.  verdict == nullptr: the PROVISIONAL sum of every tuple's
// candidates, which also writes the tuple's flag; else the RE-SUM of the tuples that go the exact way (their rows zeroed by k_clo_settle),
// under the exact call's rule — the other tuples' outputs are not touched.
KERNEL_SMALL void k_clo_sum_lane(ClShares in, size_t n, size_t bm_words, uint64_t wave_min, uint32_t min_tuple, const uint8_t* verdict, uint8_t* flag,
                                 uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  uint64_t len = verdict ? clo_resum_len(in, live ? i : 0, live, flag, verdict) : cl_tuple_len(in, live ? i : 0, live);
  const bool mine = live && len < wave_min && (!verdict || clo_goes_exact(flag[i], verdict[i]));
  if (!mine) len = 0;
  G1Jac acc;
  uint32_t count, dup;
  clo_lane_sum(acc, count, dup, bits + (mine ? i : 0) * bm_words, bm_words, in, mine ? in.off[i] : 0, len);
  G1Affine r;
  jac_to_affine(r, acc);
  if (!mine) return;
  encode_g1(agg + 64 * i, r);
  if (n_signers) n_signers[i] = count;
  if (!verdict) flag[i] = clo_flag(count, dup, min_tuple);
}
KERNEL_SMALL void k_clo_sum_wave(ClShares in, size_t n, size_t bm_words, uint64_t wave_min, uint32_t min_tuple, const uint8_t* verdict, uint8_t* flag,
                                 uint32_t* bits, uint8_t* agg, uint32_t* n_signers) {
  __shared__ ClJacSlot part[BN_WAVE];
  __shared__ uint32_t cnt[BN_WAVE], dupf[BN_WAVE];
  const unsigned t = threadIdx.x;
  for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t len = verdict ? clo_resum_len(in, i, true, flag, verdict) : cl_tuple_len(in, i, true);
    if (len < wave_min) continue;                      // wave_min >= 1: also every tuple the re-sum masks out
    clo_wave_partial(part[t].v, cnt[t], dupf[t], bits + i * bm_words, bm_words, in, in.off[i], len, t);
    __syncthreads();
    for (unsigned stride = BN_WAVE / 2; stride >= 1; stride >>= 1) {
      if (t < stride) clo_tree_level(part, cnt, dupf, t, stride);
      __syncthreads();
    }
    if (t == 0) {
      cl_encode(agg + 64 * i, part[0].v);
      if (n_signers) n_signers[i] = cnt[0];
      if (!verdict) flag[i] = clo_flag(cnt[0], dupf[0], min_tuple);
    }
    __syncthreads();
  }
}
// the tuple check's H(m): tuple base + j into slot j, as k_cl_spread gives a share its tuple's
KERNEL_SMALL void k_clo_load_h(size_t len, size_t base, ClScratch S, Ws ws) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j >= len) return;
  const int32_t* w = S.hpt + (base + j) * CL_HASH_WORDS;
  Fp x, y;
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) { x.v[k] = w[k]; y.v[k] = w[BN_LIMBS + k]; }
  ws_store_fp(ws, PL_P2X, j, x);
  ws_store_fp(ws, PL_P2Y, j, y);
  ws_byte(ws, BY_P2_INF, j) = S.hinf[base + j];
  ws_byte(ws, BY_ST_HASH, j) = S.hst[base + j];
}
// behind the tuple check: the rows of the tuples that go the exact way are zeroed for the re-sum, and the call's counters take what the
// check did (one vector atomic per wave and counter)
KERNEL_SMALL void k_clo_settle(size_t n, size_t bm_words, ClScratch S, uint32_t* bits) {
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
// slot j of a slice = share base + j: queued for the exact keyed verify iff it is a candidate of a tuple that goes the exact way
KERNEL_SMALL void k_clo_queue(size_t len, uint64_t base, size_t n, const uint64_t* off, ClScratch S, const uint8_t* share_status, Ws ws) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j >= len) return;
  const size_t t = cl_tuple_of(base + j, S.end, off, n);
  if (clo_queued(share_status[base + j], t, n, S.flag, S.verdict)) ws.h_list[atomicAdd(&ws.h_cnt[0], 1u)] = (uint32_t)j;
}
// ... and the queue's length into the call's counters
KERNEL_SMALL void k_clo_count(const uint32_t* h_cnt, uint32_t* stats) {
  if (threadIdx.x == 0 && h_cnt[0]) atomicAdd(&stats[CLO_STAT_AT + 3], h_cnt[0]);
}
// The two stages the optimistic merge runs too (bn254_host.h).  The tuple check: the call's own outputs through the bitmap verify's kernels,
// decode flags 0 (an identity aggregate is legitimate); a merge over no keys has no rows
int clo_tuple_check(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t t_piece, const ClScratch& S) {
  int rc;
  const bool tables = bm_wants_tables(c);
  for (size_t lo = 0; lo < a.n; lo += t_piece) {
    const size_t len = a.n - lo < t_piece ? a.n - lo : t_piece;
    if ((rc = launch_decode_g1(c, s, a.agg_sigs + 64 * lo, len, 0, PL_P1X, BY_P1_INF, 0))) return rc;
    k_clo_load_h<<<grid_for(len), BN_WAVE, 0, s>>>(len, lo, S, c->ws);
    HIP_TRY(hipGetLastError());
    if ((rc = launch_bitmap_sum(c, s, a.signer_bits ? a.signer_bits + lo * a.bm_words : nullptr, a.bm_words, len, tables))) return rc;
    PROF_MARK(2);
    if ((rc = launch_verify_miller_fe(c, s, len, BN_PAIRS_VERIFY, 1, S.verdict + lo, false))) return rc;
  }
  PROF_MARK(3);
  k_clo_settle<<<grid_for(a.n), BN_WAVE, 0, s>>>(a.n, a.bm_words, S, a.signer_bits);
  HIP_TRY(hipGetLastError());
  return 0;
}
// The queue holds at most len entries (one per slot), and the workspace was reserved for a slice's length
int clo_queue_slice(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t lo, size_t len, const ClScratch& S) {
  if (const int rc = launch_decode_g1(c, s, a.items + 64 * lo, len, a.flags, PL_P1X, BY_P1_INF, 0)) return rc;
  k_cl_spread<<<grid_for(len), BN_WAVE, 0, s>>>(len, (uint64_t)lo, a.n, a.off, S, c->ws);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(c->ws.h_cnt, 0, sizeof(uint32_t), s));
  k_clo_queue<<<grid_for(len), BN_WAVE, 0, s>>>(len, (uint64_t)lo, a.n, a.off, S, a.item_status, c->ws);
  HIP_TRY(hipGetLastError());
  k_clo_count<<<1, BN_WAVE, 0, s>>>(c->ws.h_cnt, S.stats);
  HIP_TRY(hipGetLastError());
  return 0;
}
// The same stages one by one, for the optimistic threshold call (bn254_threshold.hip), whose tuple check runs under the group key: rules 1-3
// of every share; H(m) of the tuples lo .. lo + len beside whatever the caller decoded into entries 0 .. len; the settle behind the verdicts
int clo_precheck_all(bn254_ctx* c, hipStream_t s, const ClCall& a, const ClScratch& S) {
  if (!a.n_items) return 0;
  k_clo_precheck<<<grid_for(a.n_items), BN_WAVE, 0, s>>>(a.n_items, a.n, a.items, a.aux, a.off, a.flags, S, c->key_st, (uint32_t)c->n_keys, a.item_status);
  HIP_TRY(hipGetLastError());
  return 0;
}
int clo_load_h(bn254_ctx* c, hipStream_t s, size_t lo, size_t len, const ClScratch& S) {
  k_clo_load_h<<<grid_for(len), BN_WAVE, 0, s>>>(len, lo, S, c->ws);
  HIP_TRY(hipGetLastError());
  return 0;
}
int clo_settle(bn254_ctx* c, hipStream_t s, const ClCall& a, const ClScratch& S) {
  (void)c;
  k_clo_settle<<<grid_for(a.n), BN_WAVE, 0, s>>>(a.n, a.bm_words, S, a.signer_bits);
  HIP_TRY(hipGetLastError());
  return 0;
}
// The route behind the hash, the range rule and the fills (cl_collect_run): pre-check, provisional sum, the tuple check in pieces of
// t_piece tuples, then the exact verify of the queued candidates in slices of s_piece shares and the re-sum.  Everything is enqueued whether
// or not a tuple fails: the host never learns.  ms[0] = front end + provisional sum, ms[1] = aggregate keys, ms[2] = the tuples' Miller loop
// and final exponentiation, ms[3] = exact fallback + re-sum (a call in several pieces: the last piece's ms[1] boundary).
static int cl_optimistic(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t t_piece, size_t s_piece, const ClScratch& S) {
  int rc;
  const size_t n = a.n, n_shares = a.n_items;
  const ClShares in = {a.items, a.aux, a.off, a.item_status, a.tuple_status};
  const uint64_t wave_min = (uint64_t)c->collect_wave_min;
  const uint32_t min_tuple = (uint32_t)c->collect_opt_min_tuple_shares;
  const unsigned wave_grid = (unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS);
  const KeyTable kt = {c->key_lines, c->key_st, c->key_inf, (uint32_t)c->n_keys};
  // 3. rules 1-3 of every share; 4. the provisional sum of the candidates and the tuples' flags
  k_clo_precheck<<<grid_for(n_shares), BN_WAVE, 0, s>>>(n_shares, n, in.shares, in.key, in.off, a.flags, S, c->key_st, (uint32_t)c->n_keys, a.item_status);
  HIP_TRY(hipGetLastError());
  k_clo_sum_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, min_tuple, nullptr, S.flag, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  k_clo_sum_wave<<<wave_grid, BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, min_tuple, nullptr, S.flag, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  PROF_MARK(1);
  // 5. the tuple check of the call's own outputs
  if ((rc = clo_tuple_check(c, s, a, t_piece, S))) return rc;
  // 6. the candidates of the tuples that go the exact way, verified by the keyed kernels over a queue; then those tuples summed again
  for (size_t lo = 0; lo < n_shares; lo += s_piece) {
    const size_t len = n_shares - lo < s_piece ? n_shares - lo : s_piece;
    if ((rc = clo_queue_slice(c, s, a, lo, len, S))) return rc;
    if ((rc = bn254_pair_miller_verify_keyed(len, c->ws, in.key + lo, kt, s, 0, c->ws.h_list, c->ws.h_cnt))) return rc;
    if ((rc = bn254_pair_final_exp(len, c->ws, 1, a.item_status + lo, c->ws.h_list, c->ws.h_cnt, s))) return rc;
  }
  k_clo_sum_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, min_tuple, S.verdict, S.flag, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  k_clo_sum_wave<<<wave_grid, BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, min_tuple, S.verdict, S.flag, a.signer_bits, a.agg_sigs, a.n_signers);
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}

// all three calls behind their checks, and the threshold call's first step: seed32 == nullptr and !optimistic is the exact one
int cl_collect_run(bn254_ctx* c, const ClCall& call, const uint8_t* seed32, bool optimistic, hipStream_t s, ClScratch* scratch) {
  ClCall a = call;
  const size_t n = a.n, n_shares = a.n_items;
  // every buffer before the first kernel: growing one waits for the context's streams, which must not happen between the steps.  The
  // tuples are hashed, and the shares verified, in pieces of the slicing rule's size; the scratch holds the whole call.
  // The randomised route when the host can tell that it pays: keys to group by, enough shares, enough of them per key (groups are per key: a
  // call whose keys have one or two shares each buys padding, not speed) — and a slice with its groups fits.  Else the exact route, same bytes.
  size_t r_piece = 0;
  if (seed32 && c->n_keys && c->key_lines && n_shares && n_shares >= (size_t)c->collect_rand_min_shares &&
      n_shares / c->n_keys >= (size_t)c->collect_rand_min_per_key)
    r_piece = cl_rand_slice_len(c, n_shares);
  if (r_piece && !cl_rand_slots_fit(c, r_piece)) r_piece = 0;
  const bool rand = r_piece != 0;
  // the optimistic route: keys to sum, and enough shares for one more verify pass to pay.  Else the exact route, same bytes.
  const bool opt = optimistic && c->n_keys && c->key_lines && n_shares && n_shares >= (size_t)c->collect_opt_min_shares;
  // the randomised call's own flags choose the weights; the remaining ones apply to the shares' decode on either route
  const int mode = rand_mode_of(a.flags);
  if (seed32) a.flags &= BN254_FLAG_G2_SUBGROUP_CHECK | BN254_FLAG_REJECT_IDENTITY;
  const size_t t_chunk = ws_chunk_for(c, n), s_chunk = n_shares && !rand ? ws_chunk_for(c, n_shares) : 0;
  const size_t t_piece = t_chunk ? t_chunk : n, s_piece = rand ? r_piece : s_chunk ? s_chunk : n_shares;
  const size_t s_entries = rand ? keyed_rand_need(c, s_piece).ws_entries : s_piece;
  int rc = ws_reserve(c, t_piece > s_entries ? t_piece : s_entries);
  if (rc) return rc;
  if (rand) {                                          // the grouping scratch of the longest slice (stage slots 5 and 7) covers every slice
    const KeyedRandNeed need = keyed_rand_need(c, s_piece);
    if ((rc = stage_reserve(c, 5, need.words * sizeof(uint32_t)))) return rc;
    if ((rc = stage_reserve(c, 7, need.groups_max))) return rc;
  }
  ClScratch& S = *scratch;
  if ((rc = cl_scratch_reserve(c, n, &S))) return rc;
  c->clr_stats = S.stats;
  c->clo_stats = S.stats + CLO_STAT_AT;
  if (opt && (rc = bm_prepare(c, s, bm_wants_tables(c)))) return rc;   // the first call after a registration builds here, ahead of the timed intervals
  RandSeed seed = {};
  if (rand) seed = rand_seed_from(seed32);
  if (rand || opt) HIP_TRY(hipMemsetAsync(S.stats, 0, CL_STAT_WORDS * sizeof(uint32_t), s));
  PROF_MARK(opt ? 0 : 1);
  // 1. hash once per tuple; 2. the range rule, the tuples' statuses, share -> tuple
  if ((rc = cl_hash_and_plan(c, s, a, t_piece, S))) return rc;
  if (a.bm_words) HIP_TRY(hipMemsetAsync(a.signer_bits, 0, n * a.bm_words * sizeof(uint32_t), s));
  if (n_shares) HIP_TRY(hipMemsetAsync(a.item_status, ST_INDEX_OOB, n_shares, s));
  if (opt) {
    if ((rc = cl_optimistic(c, s, a, t_piece, s_piece, S))) return rc;
    c->clo_last_ran = 1;
    return 0;
  }
  // 3. the keyed verify of the share slots
  for (size_t lo = 0; lo < n_shares; lo += s_piece) {
    const size_t len = n_shares - lo < s_piece ? n_shares - lo : s_piece;
    if ((rc = rand ? cl_verify_slice_rand(c, s, a, lo, len, seed, mode, S) : cl_verify_slice(c, s, a, lo, len, S))) return rc;
  }
  if (!n_shares) { PROF_MARK(2); PROF_MARK(3); PROF_MARK(4); }
  // 4. select-and-sum, once, behind the last slice
  const ClShares in = {a.items, a.aux, a.off, a.item_status, a.tuple_status};
  const uint64_t wave_min = (uint64_t)c->collect_wave_min;
  k_cl_sum_lane<<<grid_for(n), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, a.signer_bits, a.agg_sigs, a.n_signers);
  HIP_TRY(hipGetLastError());
  k_cl_sum_wave<<<(unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS), BN_WAVE, 0, s>>>(in, n, a.bm_words, wave_min, a.signer_bits, a.agg_sigs, a.n_signers);
  PROF_MARK(0);
  prof_done(c, EV_COLLECT);
  HIP_TRY(hipGetLastError());
  c->clr_last_ran = rand ? 1 : 0;                      // only a call that enqueued everything has something for the debug hook to read
  return 0;
}

// the checked entry of the three *_device calls
static int cl_collect_device(bn254_ctx* c, const ClCall& a, const uint8_t* seed32, bool optimistic, void* stream) {
  if (g1c_flag(a.flags))                                // compressed shares: staged once, in front of the hash and of any slicing
    return cl_g1c_call(c, a, stream, [&](const ClCall& d) { return cl_collect_device(c, d, seed32, optimistic, stream); });
  MsgsLenScope msgs_len_scope(c);
  if (c) c->clr_last_ran = c->clo_last_ran = c->mgo_last_ran = c->tho_last_ran = 0;
  int rc = BN254_E_BAD_ARGUMENT;
  if (!cl_keys_ok(c, a) || !cl_checks_device(c, a, &rc)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  ClScratch S;
  return cl_collect_run(c, a, seed32, optimistic, s, &S);
}
// the host-pointer form of the three.  The randomised call's grouping scratch lives in stage slots 5 and 7, so its outputs take slot 6.
static int cl_collect_host(bn254_ctx* c, const ClCall& a, const uint8_t* seed32, bool optimistic) {
  MsgsLenScope msgs_len_scope(c);
  if (c) c->clr_last_ran = c->clo_last_ran = c->mgo_last_ran = c->tho_last_ran = 0;
  int rc = BN254_E_BAD_ARGUMENT;
  if (!cl_keys_ok(c, a) || !cl_checks_host(c, a, &rc)) return rc;
  HostStaging st(c);
  ClCall d;
  cl_stage(st, a, 1, seed32 ? 6 : 5, &d);
  if (st.ok()) st.rc = cl_collect_device(c, d, seed32, optimistic, nullptr);
  return st.finish();
}

extern "C" {

int bn254_batch_collect_keyed_bitmap_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_shares,
                                            const uint32_t* d_share_key, const uint64_t* d_share_off, size_t n_shares, size_t n, size_t bm_words,
                                            uint32_t flags, uint8_t* d_share_status, uint8_t* d_tuple_status, uint8_t* d_agg_sigs,
                                            uint32_t* d_signer_bits, uint32_t* d_n_signers, void* stream) {
  const ClCall a = {.msgs = d_msgs, .msg_off = d_msg_off, .items = d_shares, .aux = d_share_key, .off = d_share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = d_share_status, .tuple_status = d_tuple_status, .agg_sigs = d_agg_sigs,
                    .signer_bits = d_signer_bits, .n_signers = d_n_signers};
  return cl_collect_device(c, a, nullptr, false, stream);
}
int bn254_batch_collect_keyed_bitmap(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* shares, const uint32_t* share_key,
                                     const uint64_t* share_off, size_t n_shares, size_t n, size_t bm_words, uint32_t flags, uint8_t* share_status,
                                     uint8_t* tuple_status, uint8_t* agg_sigs, uint32_t* signer_bits, uint32_t* n_signers) {
  const ClCall a = {.msgs = msgs, .msg_off = msg_off, .items = shares, .aux = share_key, .off = share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = share_status, .tuple_status = tuple_status, .agg_sigs = agg_sigs,
                    .signer_bits = signer_bits, .n_signers = n_signers};
  return cl_collect_host(c, a, nullptr, false);
}
int bn254_batch_collect_keyed_bitmap_randomized_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_shares,
                                                       const uint32_t* d_share_key, const uint64_t* d_share_off, size_t n_shares, size_t n,
                                                       size_t bm_words, uint32_t flags, const uint8_t* seed32, uint8_t* d_share_status,
                                                       uint8_t* d_tuple_status, uint8_t* d_agg_sigs, uint32_t* d_signer_bits, uint32_t* d_n_signers,
                                                       void* stream) {
  if (!seed32) return BN254_E_BAD_ARGUMENT;
  const ClCall a = {.msgs = d_msgs, .msg_off = d_msg_off, .items = d_shares, .aux = d_share_key, .off = d_share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = d_share_status, .tuple_status = d_tuple_status, .agg_sigs = d_agg_sigs,
                    .signer_bits = d_signer_bits, .n_signers = d_n_signers};
  return cl_collect_device(c, a, seed32, false, stream);
}
int bn254_batch_collect_keyed_bitmap_randomized(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* shares,
                                                const uint32_t* share_key, const uint64_t* share_off, size_t n_shares, size_t n, size_t bm_words,
                                                uint32_t flags, const uint8_t* seed32, uint8_t* share_status, uint8_t* tuple_status, uint8_t* agg_sigs,
                                                uint32_t* signer_bits, uint32_t* n_signers) {
  if (!seed32) return BN254_E_BAD_ARGUMENT;
  const ClCall a = {.msgs = msgs, .msg_off = msg_off, .items = shares, .aux = share_key, .off = share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = share_status, .tuple_status = tuple_status, .agg_sigs = agg_sigs,
                    .signer_bits = signer_bits, .n_signers = n_signers};
  return cl_collect_host(c, a, seed32, false);
}
int bn254_batch_collect_keyed_bitmap_optimistic_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_msg_off, const uint8_t* d_shares,
                                                       const uint32_t* d_share_key, const uint64_t* d_share_off, size_t n_shares, size_t n,
                                                       size_t bm_words, uint32_t flags, uint8_t* d_share_status, uint8_t* d_tuple_status,
                                                       uint8_t* d_agg_sigs, uint32_t* d_signer_bits, uint32_t* d_n_signers, void* stream) {
  const ClCall a = {.msgs = d_msgs, .msg_off = d_msg_off, .items = d_shares, .aux = d_share_key, .off = d_share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = d_share_status, .tuple_status = d_tuple_status, .agg_sigs = d_agg_sigs,
                    .signer_bits = d_signer_bits, .n_signers = d_n_signers};
  return cl_collect_device(c, a, nullptr, true, stream);
}
int bn254_batch_collect_keyed_bitmap_optimistic(bn254_ctx* c, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* shares,
                                                const uint32_t* share_key, const uint64_t* share_off, size_t n_shares, size_t n, size_t bm_words,
                                                uint32_t flags, uint8_t* share_status, uint8_t* tuple_status, uint8_t* agg_sigs,
                                                uint32_t* signer_bits, uint32_t* n_signers) {
  const ClCall a = {.msgs = msgs, .msg_off = msg_off, .items = shares, .aux = share_key, .off = share_off, .n_items = n_shares, .n = n,
                    .bm_words = bm_words, .flags = flags, .item_status = share_status, .tuple_status = tuple_status, .agg_sigs = agg_sigs,
                    .signer_bits = signer_bits, .n_signers = n_signers};
  return cl_collect_host(c, a, nullptr, true);
}

}  // extern "C"
