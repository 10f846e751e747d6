// Translation unit of libbn254hip.so: t-of-n threshold signatures over the registered keys and the segmented scalar-weighted sum in G1
// (include/bn254_hip.h: bn254_batch_threshold_combine_keyed[_device], bn254_batch_g1_msm[_device]).  The threshold call IS
// the exact collect (bn254_collect.hip: cl_collect_run, behind the family's shared checks and staging — bn254_host.h: ClCall: front end, range
// rule, keyed verify slices, claim pass) followed by rank-and-select on the rows it left, one Lagrange coefficient per kept key, and the
// term and sum kernels of the weighted sum.  The bookkeeping and the arithmetic are bn254_threshold.h and bn254_fr.h, shared with the CPU
// suite's host compilation.
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
static int th_scratch_reserve(bn254_ctx* c, size_t items, size_t claim_words, bool coefficients, ThScratch* T) {
  Carve size(nullptr);
  th_scratch(size, items, claim_words, coefficients);
  if (const int rc = scratch_reserve(c, &c->th_buf, &c->th_cap, size.used)) return rc;
  Carve carve(c->th_buf);
  *T = th_scratch(carve, items, claim_words, coefficients);
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
  c->clr_last_ran = c->clo_last_ran = c->mgo_last_ran = 0;
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

}  // extern "C"
