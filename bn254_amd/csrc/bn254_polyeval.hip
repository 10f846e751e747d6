// Translation unit of libbn254hip.so: polynomials with G2 coefficients evaluated at small integer points, and the registration of the share keys
// of a vector of Feldman commitments (include/bn254_hip.h: bn254_batch_g2_poly_eval[_device], bn254_ctx_register_keys_commitments; DESIGN.md
// §10n).  Three kernels: the coefficients are decoded ONCE into scratch (a lane each); an evaluation of a polynomial shorter than
// BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS is one lane's Horner walk, acc <- x acc + C_k with a double-and-add by the small x; a longer one is a
// wave's: 64 chunks, each partial multiplied by its power of x through the 256-step ladder and the 64 products folded by the sums' six-level
// tree in LDS.  The registration runs the evaluation at x = 1 .. n_keys and hands its output, still in device memory, to the kernel every
// registration runs.  The arithmetic and the bookkeeping are bn254_polyeval.h, shared with the CPU suite's host compilation.
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

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"
#include "bn254_aggd_plan.h"

// per coefficient: 4 x 9 Montgomery limbs, the identity byte and the decode status (146 B); for the registration also the evaluations it makes
// up itself — polynomial 0 at x = 1 .. n —, their 128-byte outputs and statuses, and the two offsets of the one polynomial
struct PeScratch {
  int32_t* xy;
  uint64_t* off;
  uint32_t *eval_poly, *eval_x;
  uint8_t *out, *inf, *st, *eval_st;
};
static PeScratch pe_scratch(Carve& c, size_t m, size_t n_reg) {
  PeScratch b;
  b.off = c.take<uint64_t>(n_reg ? 2 : 0);
  b.xy = c.take<int32_t>(m * PE_COEFF_WORDS);
  b.eval_poly = c.take<uint32_t>(n_reg), b.eval_x = c.take<uint32_t>(n_reg);
  b.out = (uint8_t*)c.take<uint32_t>(n_reg * 32);
  b.inf = c.take<uint8_t>(m), b.st = c.take<uint8_t>(m), b.eval_st = c.take<uint8_t>(n_reg);
  return b;
}
static int pe_scratch_reserve(bn254_ctx* c, size_t m, size_t n_reg, PeScratch* P) {
  Carve size(nullptr);
  pe_scratch(size, m, n_reg);
  if (const int rc = scratch_reserve(c, &c->th_buf, &c->th_cap, size.used)) return rc;
  Carve carve(c->th_buf);
  *P = pe_scratch(carve, m, n_reg);
  return 0;
}

// what an evaluation reads: the decoded coefficients and the caller's three arrays
struct PeIn {
  const int32_t* xy;
  const uint8_t *inf, *st;
  const uint64_t* poly_off;
  const uint32_t *eval_poly, *eval_x;
  uint64_t p, m;
};

// one lane per coefficient.  A lane past the end decodes coefficient 0 and writes nothing, so the wave stays convergent through the decoder
KERNEL_SMALL void k_pe_decode(const uint8_t* coeffs, size_t m, int32_t* xy, uint8_t* inf, uint8_t* st) {
  const size_t s = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = s < m;
  int32_t w[PE_COEFF_WORDS];
  uint8_t i, t;
  pe_decode(w, i, t, coeffs + 128 * (live ? s : 0));
  if (!live) return;
#pragma unroll
  for (int k = 0; k < PE_COEFF_WORDS; ++k) xy[s * PE_COEFF_WORDS + k] = w[k];
  inf[s] = i;
  st[s] = t;
}
// the registration's evaluations: polynomial 0 = all t coefficients, at x = j + 1
KERNEL_SMALL void k_pe_share_points(uint32_t t, size_t n, uint64_t* off, uint32_t* eval_poly, uint32_t* eval_x) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j == 0) { off[0] = 0; off[1] = t; }
  if (j >= n) return;
  eval_poly[j] = 0;
  eval_x[j] = (uint32_t)j + 1u;
}
// the largest value any lane of the wave holds
__device__ __forceinline__ uint32_t pe_wave_max(uint32_t v) {
#pragma unroll
  for (int o = BN_WAVE / 2; o >= 1; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)v, o, BN_WAVE);
    v = other > v ? other : v;
  }
  return v;
}
// lane per evaluation: the polynomials below wave_min coefficients, and the refused ones, which have none.  No early return in front of the
// votes of the additions but the wave-uniform one; a lane that is not its evaluation's walks the empty polynomial at x = 0
KERNEL void k_pe_eval_lane(PeIn in, size_t q, uint64_t wave_min, uint8_t* out, uint8_t* status) {
  const size_t e = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = e < q;
  uint64_t lo = 0;
  uint8_t span_st = ST_OK;
  uint64_t len = live ? pe_span(in.poly_off, in.p, in.m, in.eval_poly[e], lo, span_st) : 0;
  const bool mine = live && (span_st != ST_OK || len < wave_min);
  if (!mine) len = 0;
  if (!BN_WAVE_ANY(mine)) return;
  const uint32_t x = mine ? in.eval_x[e] : 0;
  const uint64_t max_len = pe_wave_max((uint32_t)len);          // len <= m < 2^32
  const int bits = (int)pe_wave_max((uint32_t)pe_bits(x));
  G2Jac acc;
  uint8_t st;
  pe_lane_eval(acc, st, x, in.xy, in.inf, in.st, lo, len, max_len, bits);
  if (span_st != ST_OK) st = span_st;
  G2Affine r;
  jac_to_affine(r, acc);
  if (!mine) return;
  if (st != ST_OK) r.inf = true;
  encode_g2(out + 128 * e, r);
  status[e] = st;
}
// wave per evaluation, the others.  LDS per workgroup (one wave) as k_g2msm_sum_wave: 64 slots of 220 B, counts, indices and statuses, 14 912 B;
// one wave per SIMD (at two the tree's additions spilled), four workgroups to a CU
KERNEL void k_pe_eval_wave(PeIn in, size_t q, uint64_t wave_min, uint8_t* out, uint8_t* status) {
  __shared__ G2JacSlot part[BN_WAVE];
  __shared__ uint32_t cnt[BN_WAVE];
  __shared__ uint64_t bad[BN_WAVE];
  __shared__ uint8_t st[BN_WAVE];
  const unsigned t = threadIdx.x;
  for (size_t e = blockIdx.x; e < q; e += gridDim.x) {
    uint64_t lo;
    uint8_t span_st;
    const uint64_t len = pe_span(in.poly_off, in.p, in.m, in.eval_poly[e], lo, span_st);
    if (span_st != ST_OK || len < wave_min) continue;   // wave-uniform
    const uint32_t x = in.eval_x[e];
    G2Jac partial;
    pe_wave_partial(partial, st[t], bad[t], x, in.xy, in.inf, in.st, lo, len, t);
    pe_wave_scale(part[t].v, partial, x, len, t);
    cnt[t] = 1;
    __syncthreads();
    for (unsigned stride = BN_WAVE / 2; stride >= 1; stride >>= 1) {
      if (t < stride) msm_tree_level(part, cnt, st, bad, t, stride);
      __syncthreads();
    }
    if (t == 0) {
      g2msm_encode(out + 128 * e, part[0].v, st[0]);
      status[e] = st[0];
    }
    __syncthreads();
  }
}
// the decode alone, for the unit that combines vectors (bn254_host.h; bn254_reshare.hip): m points into the 146 B layout, enqueued on s
int launch_pe_decode(hipStream_t s, const uint8_t* d_points, size_t m, int32_t* xy, uint8_t* inf, uint8_t* st) {
  if (m == 0) return 0;
  k_pe_decode<<<grid_for(m), BN_WAVE, 0, s>>>(d_points, m, xy, inf, st);
  HIP_TRY(hipGetLastError());
  return 0;
}
// decode and both layouts, enqueued on s; P holds m coefficients
static int launch_poly_eval(bn254_ctx* c, hipStream_t s, const uint8_t* d_coeffs, size_t m, const uint64_t* d_poly_off, size_t p, const uint32_t* d_eval_poly,
                            const uint32_t* d_eval_x, size_t q, const PeScratch& P, uint8_t* d_out, uint8_t* d_status) {
  if (m) {
    k_pe_decode<<<grid_for(m), BN_WAVE, 0, s>>>(d_coeffs, m, P.xy, P.inf, P.st);
    HIP_TRY(hipGetLastError());
  }
  const PeIn in = {P.xy, P.inf, P.st, d_poly_off, d_eval_poly, d_eval_x, (uint64_t)p, (uint64_t)m};
  const uint64_t wave_min = (uint64_t)c->pe_wave_min;
  k_pe_eval_lane<<<grid_for(q), BN_WAVE, 0, s>>>(in, q, wave_min, d_out, d_status);
  HIP_TRY(hipGetLastError());
  k_pe_eval_wave<<<(unsigned)(q < CL_WAVE_MAX_BLOCKS ? q : CL_WAVE_MAX_BLOCKS), BN_WAVE, 0, s>>>(in, q, wave_min, d_out, d_status);
  HIP_TRY(hipGetLastError());
  return 0;
}
// the _device form behind its argument checks, the number of coefficients known
static int poly_eval_device(bn254_ctx* c, const uint8_t* d_coeffs, size_t m, const uint64_t* d_poly_off, size_t p, const uint32_t* d_eval_poly,
                            const uint32_t* d_eval_x, size_t q, uint8_t* d_out, uint8_t* d_status, hipStream_t s) {
  if (m > 0xFFFFFFFFu || (m && !d_coeffs)) return BN254_E_BAD_ARGUMENT;
  PeScratch P;
  if (const int rc = pe_scratch_reserve(c, m, 0, &P)) return rc;
  CallDone call_done(c, s);
  return launch_poly_eval(c, s, d_coeffs, m, d_poly_off, p, d_eval_poly, d_eval_x, q, P, d_out, d_status);
}
// what both forms refuse before anything else.  p == 0 is legal: every evaluation then names a polynomial that is not there
static bool poly_eval_args_ok(const bn254_ctx* c, const uint64_t* poly_off, size_t p, const uint32_t* eval_poly, const uint32_t* eval_x, size_t q,
                              const uint8_t* out, const uint8_t* status) {
  return c && p <= 0xFFFFFFFFu && q <= 0xFFFFFFFFu && (p == 0 || poly_off) && (q == 0 || (eval_poly && eval_x && out && status));
}

extern "C" {

int bn254_batch_g2_poly_eval_device(bn254_ctx* c, const uint8_t* d_coeffs, const uint64_t* d_poly_off, size_t p, const uint32_t* d_eval_poly,
                                    const uint32_t* d_eval_x, size_t q, uint8_t* d_out, uint8_t* d_status, void* stream) {
  if (!poly_eval_args_ok(c, d_poly_off, p, d_eval_poly, d_eval_x, q, d_out, d_status)) return BN254_E_BAD_ARGUMENT;
  if (q == 0) return 0;
  if (misaligned(d_coeffs) || misaligned(d_eval_poly) || misaligned(d_eval_x) || misaligned(d_out) || ((uintptr_t)d_poly_off & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the number of coefficients is d_poly_off[p], which sizes the scratch: one 8-byte copy home and a wait for the stream (include/bn254_hip.h)
  uint64_t m = 0;
  if (p) {
    HIP_TRY(hipMemcpyAsync(&m, d_poly_off + p, sizeof m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return poly_eval_device(c, d_coeffs, (size_t)m, d_poly_off, p, d_eval_poly, d_eval_x, q, d_out, d_status, s);
}
int bn254_batch_g2_poly_eval(bn254_ctx* c, const uint8_t* coeffs, const uint64_t* poly_off, size_t p, const uint32_t* eval_poly, const uint32_t* eval_x,
                             size_t q, uint8_t* out, uint8_t* status) {
  if (!poly_eval_args_ok(c, poly_off, p, eval_poly, eval_x, q, out, status)) return BN254_E_BAD_ARGUMENT;
  if (q == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (p && !offsets_ok(poly_off, p)) return BN254_E_BAD_ARGUMENT;
  const size_t m = p ? (size_t)poly_off[p] : 0;
  if (m && !coeffs) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_coeffs = st.in(0, coeffs, m * 128), *d_off = st.in(1, poly_off, p ? (p + 1) * sizeof(uint64_t) : 0);
  const uint8_t *d_eval_poly = st.in(2, eval_poly, q * sizeof(uint32_t)), *d_eval_x = st.in(5, eval_x, q * sizeof(uint32_t));
  uint8_t *d_out = st.out(3, q * 128, out), *d_status = st.out(4, q, status);
  if (st.ok())
    st.rc = poly_eval_device(c, d_coeffs, m, (const uint64_t*)d_off, p, (const uint32_t*)d_eval_poly, (const uint32_t*)d_eval_x, q, d_out, d_status, c->stream);
  return st.finish();
}

// host-synchronous, like every registration: the evaluation's output never leaves the device — launch_register_keys reads it where it lies
int bn254_ctx_register_keys_commitments(bn254_ctx* c, const uint8_t* commitments, uint32_t t, size_t n_keys, uint32_t flags, uint8_t* key_status,
                                        uint8_t* status) {
  if (!c || !commitments || !status || t == 0 || n_keys == 0 || n_keys > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = register_keys_begin(c, n_keys); if (rc_) return rc_; }
  PeScratch P;
  if (const int rc = pe_scratch_reserve(c, t, n_keys, &P)) return rc;
  hipStream_t s = c->stream;
  // the verdict decides whether key_status is written at all, so the key statuses wait in a buffer of the call's own
  uint8_t* key_st_home = (uint8_t*)malloc(n_keys);
  if (!key_st_home) return BN254_E_NO_MEMORY;
  uint8_t verdict = 0xFF;
  int rc = 0;
  {
    HostStaging st(c);
    const uint8_t* d_commitments = st.in(3, commitments, (size_t)t * 128);
    st.copy_back(&verdict, P.eval_st, 1);            // every evaluation reads the one polynomial: the first decode fault in coefficient order
    st.copy_back(key_st_home, c->key_st, n_keys);
    if (st.ok()) {
      k_pe_share_points<<<grid_for(n_keys), BN_WAVE, 0, s>>>(t, n_keys, P.off, P.eval_poly, P.eval_x);
      st.check(hipGetLastError());
    }
    if (st.ok()) st.rc = launch_poly_eval(c, s, d_commitments, t, P.off, 1, P.eval_poly, P.eval_x, n_keys, P, P.out, P.eval_st);
    if (st.ok()) st.rc = launch_register_keys(c, P.out, n_keys, flags);
    rc = st.finish();
  }
  if (!rc) {
    *status = verdict;
    if (verdict == ST_OK) {
      if (key_status) memcpy(key_status, key_st_home, n_keys);
      c->n_keys = n_keys;
    }
  }
  free(key_st_home);
  return rc;
}

}  // extern "C"
