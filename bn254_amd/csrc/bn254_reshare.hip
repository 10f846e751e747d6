// Translation unit of libbn254hip.so: vectors of G2 points combined column by column, one scalar per vector, and the reshare of a threshold
// key — the commitments of the next committee's polynomial from the sub-dealings of the old members (include/bn254_hip.h:
// bn254_batch_g2_vector_combine[_device], bn254_ctx_reshare_commitments).  The points are decoded ONCE by the decode of
// bn254_polyeval.hip; a term kernel walks the 256-step ladder over the decoded limbs in column-major term order, so that the terms of one
// output are one segment of the two sum kernels of bn254_dealing.hip, which run as they stand.  The reshare puts four small kernels in
// between: the dealers' statuses against the registered set, the ranking that picks the t lowest qualified ones, their Lagrange
// coefficients, and the offsets and gates of the sums.  The arithmetic and the bookkeeping are bn254_reshare.h, shared with the CPU suite's
// host compilation.
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
#include "bn254_dealing.h"
#include "bn254_polyeval.h"
#include "bn254_reshare.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"
#include "bn254_aggd_plan.h"

// per point: 4 x 9 Montgomery limbs, the identity byte and the decode status (146 B); per term: the ladder's Jacobian result and its status
// (217 B); per output: its offset, and for the reshare its gate, its 128 bytes and its status.  The reshare also holds, per dealer, the
// position taken at each rank, the coefficient (32 B big-endian) and the status; the used row; and the bytes the kernels hand each other
// and the host: |Q|, the stop byte, the call's status
struct VcScratch {
  int32_t* xy;
  G2Jac* terms;
  uint64_t* seg;
  uint32_t *pick, *row, *count;
  uint8_t *scalars, *out, *inf, *st, *term_st, *gate, *sum_st, *dealer_st, *skip, *status;
};
static VcScratch vc_scratch(Carve& c, size_t points, size_t terms, size_t len, size_t d_reshare, size_t bm_words) {
  VcScratch b;
  const size_t rs_len = d_reshare ? len : 0;
  b.terms = c.take<G2Jac>(terms);
  b.seg = c.take<uint64_t>(len + 1);
  b.xy = c.take<int32_t>(points * PE_COEFF_WORDS);
  b.pick = c.take<uint32_t>(d_reshare), b.row = c.take<uint32_t>(d_reshare ? bm_words : 0), b.count = c.take<uint32_t>(d_reshare ? 1 : 0);
  b.scalars = (uint8_t*)c.take<uint32_t>(d_reshare * 8);
  b.out = (uint8_t*)c.take<uint32_t>(rs_len * 32);
  b.inf = c.take<uint8_t>(points), b.st = c.take<uint8_t>(points), b.term_st = c.take<uint8_t>(terms);
  b.gate = c.take<uint8_t>(rs_len), b.sum_st = c.take<uint8_t>(rs_len), b.dealer_st = c.take<uint8_t>(d_reshare);
  b.skip = c.take<uint8_t>(d_reshare ? 1 : 0), b.status = c.take<uint8_t>(d_reshare ? 1 : 0);
  return b;
}
static int vc_scratch_reserve(bn254_ctx* c, size_t points, size_t terms, size_t len, size_t d_reshare, size_t bm_words, VcScratch* V) {
  Carve size(nullptr);
  vc_scratch(size, points, terms, len, d_reshare, bm_words);
  if (const int rc = scratch_reserve(c, &c->th_buf, &c->th_cap, size.used)) return rc;
  Carve carve(c->th_buf);
  *V = vc_scratch(carve, points, terms, len, d_reshare, bm_words);
  return 0;
}

// what a term reads: the decoded points (vector-major, len each), the scalars (32 B per vector), and which vectors are taken
struct VcIn {
  const int32_t* xy;
  const uint8_t *inf, *st, *scalars;
  const uint32_t* pick;
  uint64_t T, len;
};

// one lane per term s = k T + r, column-major.  No early return past the stop byte: the ladder's additions vote across the wave; a lane past
// the end walks the identity.  skip: a device byte, non-zero = too few dealers qualified (wave-uniform: every lane leaves)
KERNEL void k_vc_term(VcIn in, size_t m, int reduce, const uint8_t* skip, G2Jac* terms, uint8_t* term_st) {
  if (skip && *skip) return;
  const size_t s = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = s < m;
  G2Jac t;
  uint8_t st;
  vc_term(t, st, in.xy, in.inf, in.st, in.scalars, in.pick, in.T, in.len, s, reduce != 0, live);
  if (!live) return;
  terms[s] = t;
  term_st[s] = st;
}
// the offsets of the len segments of T terms; with a stop byte also every gate, and behind a raised one the outputs the sums then leave
// alone: zero bytes, status 0
KERNEL_SMALL void k_vc_seg(uint64_t T, size_t len, const uint8_t* skip, uint64_t* seg, uint8_t* gate, uint8_t* out, uint8_t* sum_st) {
  const size_t k = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (k > len) return;
  seg[k] = (uint64_t)k * T;
  if (!skip || k == len) return;
  const uint8_t stop = *skip;
  gate[k] = stop;
  if (!stop) return;
  uint32_t* w = (uint32_t*)(out + 128 * k);
  for (int j = 0; j < 32; ++j) w[j] = 0;
  sum_st[k] = ST_OK;
}
// a lane per dealer: rules 1 to 5 over the decoded statuses and the registered table
KERNEL_SMALL void k_rs_qualify(const int32_t* xy, const uint8_t* inf, const uint8_t* st, uint64_t len, const uint32_t* dealer_key, size_t d, const int32_t* key_xy,
                               const uint8_t* key_st, const uint8_t* key_inf, uint64_t n_keys, uint8_t* dealer_st) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= d) return;
  dealer_st[i] = rs_qualify(xy, inf, st, len, dealer_key, i, key_xy, key_st, key_inf, n_keys);
}
// one wave: the ranks of the qualified dealers by a chunked scan; pick, the used row (zeroed by the host's memset in front), |Q|, the stop
// byte and the call's status
KERNEL_SMALL void k_rs_select(const uint32_t* dealer_key, const uint8_t* dealer_st, size_t d, uint32_t t, uint32_t* pick, uint32_t* row, size_t bm_words,
                              uint32_t* count, uint8_t* skip, uint8_t* status) {
  __shared__ uint32_t part[BN_WAVE];
  __shared__ uint32_t total;
  const unsigned l = threadIdx.x;
  part[l] = rs_count(dealer_st, d, l);
  __syncthreads();
  if (l == 0) {
    total = rs_prefix(part);
    *count = total;
    rs_verdict(*skip, *status, total, t);
  }
  __syncthreads();
  rs_select_lane(pick, row, bm_words, dealer_key, dealer_st, d, l, part[l], total, t);
}
// a lane per taken dealer
KERNEL_SMALL void k_rs_coeff(const uint32_t* pick, const uint32_t* dealer_key, const uint32_t* row, size_t bm_words, uint32_t t, const uint8_t* skip, uint8_t* scalars) {
  if (*skip) return;
  const size_t r = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (r >= t) return;
  rs_coeff(scalars, pick, dealer_key, row, bm_words, r);
}

// terms and sums behind the decode, enqueued on s: T vectors taken (pick: which; null = all, in order), len outputs
static int launch_vc_terms_sums(bn254_ctx* c, hipStream_t s, const VcScratch& V, const uint8_t* d_scalars, const uint32_t* d_pick, size_t T, size_t len, int reduce,
                                const uint8_t* d_skip, uint8_t* d_out, uint8_t* d_status) {
  const size_t m = T * len;
  k_vc_seg<<<grid_for(len + 1), BN_WAVE, 0, s>>>((uint64_t)T, len, d_skip, V.seg, V.gate, d_out, d_status);
  HIP_TRY(hipGetLastError());
  if (m) {
    const VcIn in = {V.xy, V.inf, V.st, d_scalars, d_pick, (uint64_t)T, (uint64_t)len};
    k_vc_term<<<grid_for(m), BN_WAVE, 0, s>>>(in, m, reduce, d_skip, V.terms, V.term_st);
    HIP_TRY(hipGetLastError());
  }
  return launch_g2msm_sums(c, s, V.terms, V.term_st, m, V.seg, d_skip ? V.gate : nullptr, len, d_out, d_status);
}
// the _device form behind its argument checks
static int vc_device(bn254_ctx* c, const uint8_t* d_vectors, const uint8_t* d_scalars, size_t d, size_t len, int reduce, uint8_t* d_out, uint8_t* d_status,
                     hipStream_t s) {
  VcScratch V;
  if (const int rc = vc_scratch_reserve(c, d * len, d * len, len, 0, 0, &V)) return rc;
  CallDone call_done(c, s);
  if (const int rc = launch_pe_decode(s, d_vectors, d * len, V.xy, V.inf, V.st)) return rc;
  return launch_vc_terms_sums(c, s, V, d_scalars, nullptr, d, len, reduce, nullptr, d_out, d_status);
}
// what both forms refuse before anything else, and (len == 0) what they have nothing to do for.  d == 0 is legal: every sum is then empty
static int vc_args(const bn254_ctx* c, const uint8_t* vectors, const uint8_t* scalars, size_t d, size_t len, const uint8_t* out, const uint8_t* status, bool* done) {
  *done = true;
  if (!c || len > 0xFFFFFFFFu || (len && (!out || !status))) return BN254_E_BAD_ARGUMENT;
  if (len == 0) return 0;
  if (d > 0xFFFFFFFFu || d * len > 0xFFFFFFFFu || (d && (!vectors || !scalars))) return BN254_E_BAD_ARGUMENT;
  *done = false;
  return 0;
}

extern "C" {

int bn254_batch_g2_vector_combine_device(bn254_ctx* c, const uint8_t* d_vectors, const uint8_t* d_scalars, size_t d, size_t len, int reduce_scalar, uint8_t* d_out,
                                         uint8_t* d_status, void* stream) {
  bool done;
  const int rc = vc_args(c, d_vectors, d_scalars, d, len, d_out, d_status, &done);
  if (done) return rc;
  if (misaligned(d_vectors) || misaligned(d_scalars) || misaligned(d_out)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  return vc_device(c, d_vectors, d_scalars, d, len, reduce_scalar, d_out, d_status, stream ? (hipStream_t)stream : c->stream);
}
int bn254_batch_g2_vector_combine(bn254_ctx* c, const uint8_t* vectors, const uint8_t* scalars, size_t d, size_t len, int reduce_scalar, uint8_t* out,
                                  uint8_t* status) {
  bool done;
  const int rc = vc_args(c, vectors, scalars, d, len, out, status, &done);
  if (done) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t *d_vectors = st.in(0, vectors, d * len * 128), *d_scalars = st.in(1, scalars, d * 32);
  uint8_t *d_out = st.out(3, len * 128, out), *d_status = st.out(4, len, status);
  if (st.ok()) st.rc = vc_device(c, d_vectors, d_scalars, d, len, reduce_scalar, d_out, d_status, c->stream);
  return st.finish();
}

// host-synchronous, like bn254_ctx_check_dealing: the context is quiesced first, the outputs are written when the call returns
int bn254_ctx_reshare_commitments(bn254_ctx* c, const uint8_t* vectors, const uint32_t* dealer_key, size_t d, uint32_t t_new, uint32_t threshold, uint32_t flags,
                                  uint8_t* dealer_status, uint32_t* used_bits, size_t bm_words, uint8_t* commitments, uint8_t* status) {
  if (!c || !vectors || !dealer_key || !dealer_status || !used_bits || !commitments || !status) return BN254_E_BAD_ARGUMENT;
  if (d == 0 || t_new == 0 || threshold == 0 || flags != 0 || c->n_keys == 0 || bm_words < (c->n_keys + 31) / 32) return BN254_E_BAD_ARGUMENT;
  if (d > 0xFFFFFFFFu || d * (size_t)t_new > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  for (size_t i = 1; i < d; ++i)
    if (dealer_key[i - 1] >= dealer_key[i]) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  const size_t len = t_new;
  // fewer dealers or keys than the threshold: too few can qualify, no term is walked (the ranking still leaves Q in the row)
  const size_t T = (threshold > d || threshold > c->n_keys) ? 0 : threshold;
  VcScratch V;
  if (const int rc = vc_scratch_reserve(c, d * len, T * len, len, d, bm_words, &V)) return rc;
  hipStream_t s = c->stream;
  HostStaging st(c);
  const uint8_t* d_vectors = st.in(0, vectors, d * len * 128);
  const uint32_t* d_keys = (const uint32_t*)st.in(1, dealer_key, d * sizeof(uint32_t));
  st.copy_back(dealer_status, V.dealer_st, d);
  st.copy_back(used_bits, V.row, bm_words * sizeof(uint32_t));
  st.copy_back(commitments, V.out, len * 128);
  st.copy_back(status, V.status, 1);
  if (!st.ok()) return st.rc;
  HIP_TRY(hipMemsetAsync(V.row, 0, bm_words * sizeof(uint32_t), s));
  if (const int rc = launch_pe_decode(s, d_vectors, d * len, V.xy, V.inf, V.st)) return rc;
  k_rs_qualify<<<grid_for(d), BN_WAVE, 0, s>>>(V.xy, V.inf, V.st, (uint64_t)len, d_keys, d, c->key_xy, c->key_st, c->key_inf, (uint64_t)c->n_keys, V.dealer_st);
  HIP_TRY(hipGetLastError());
  k_rs_select<<<1, BN_WAVE, 0, s>>>(d_keys, V.dealer_st, d, threshold, V.pick, V.row, bm_words, V.count, V.skip, V.status);
  HIP_TRY(hipGetLastError());
  if (T) {
    k_rs_coeff<<<grid_for(T), BN_WAVE, 0, s>>>(V.pick, d_keys, V.row, bm_words, threshold, V.skip, V.scalars);
    HIP_TRY(hipGetLastError());
  }
  if (const int rc = launch_vc_terms_sums(c, s, V, V.scalars, V.pick, T, len, 0, V.skip, V.out, V.sum_st)) return rc;
  return st.finish();
}

}  // extern "C"
