// Translation unit of libbn254hip.so: the segmented scalar-weighted sum in G2 and the check of a t-of-n dealing over the registered keys
// (include/bn254_hip.h: bn254_batch_g2_msm[_device], bn254_ctx_check_dealing, bn254_debug_dealing_coefficients).  The sum is
// the G1 sum's shape (bn254_threshold.hip) over G2Jac: a term kernel — the 256-step ladder of bn254_batch_g2_mul, one lane per term, no
// inversion — and the segment sums in the collect's two layouts.  The check derives, from a seed, coefficients c_j with sum_j c_j f(x_j) = 0
// for every polynomial f of degree below the threshold (Fr on the device, factorial closed forms for the consecutive points x_j = j + 1), and
// runs the group key sum_k lambda_k pk_k and the check sum_j c_j pk_j as ONE launch of the sum's kernels over two segments whose terms read
// the registered table instead of decoding bytes; a last kernel settles the verdict.  The arithmetic and the bookkeeping are
// bn254_dealing.h, bn254_threshold.h and bn254_fr.h, shared with the CPU suite's host compilation.
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

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"
#include "bn254_aggd_plan.h"

// per term: the ladder's Jacobian result and the point's decode status; for the check also the tables of the coefficients (n + 1 factorials and
// inverses, n - t weights), the scalars of the t + n terms (32 B big-endian), and the few words the kernels hand each other: the two
// segments' offsets, encodings and statuses, the lowest refused key, the byte that stops every kernel behind it, the result
struct DlScratch {
  G2Jac* terms;
  Fr *fact, *inv, *w;
  uint64_t* seg;
  DlResult* result;
  uint32_t* bad_key;
  uint8_t *scalars, *sums, *term_st, *sum_st, *gate, *bad_st, *skip;
};
static DlScratch dl_scratch(Carve& c, size_t terms, size_t n, size_t t, bool check) {
  DlScratch b;
  b.terms = c.take<G2Jac>(terms);
  b.fact = c.take<Fr>(check ? n + 1 : 0), b.inv = c.take<Fr>(check ? n + 1 : 0), b.w = c.take<Fr>(check ? n - t : 0);
  b.seg = c.take<uint64_t>(check ? 3 : 0);
  b.result = c.take<DlResult>(check ? 1 : 0);
  b.bad_key = c.take<uint32_t>(check ? 1 : 0);
  b.scalars = (uint8_t*)c.take<uint32_t>(check ? (t + n) * 8 : 0);
  b.sums = (uint8_t*)c.take<uint32_t>(check ? 64 : 0);
  b.term_st = c.take<uint8_t>(terms);
  b.sum_st = c.take<uint8_t>(check ? 2 : 0), b.gate = c.take<uint8_t>(check ? 2 : 0), b.bad_st = c.take<uint8_t>(check ? 1 : 0), b.skip = c.take<uint8_t>(check ? 1 : 0);
  return b;
}
static int dl_scratch_reserve(bn254_ctx* c, size_t terms, size_t n, size_t t, bool check, DlScratch* D) {
  Carve size(nullptr);
  dl_scratch(size, terms, n, t, check);
  if (const int rc = scratch_reserve(c, &c->th_buf, &c->th_cap, size.used)) return rc;
  Carve carve(c->th_buf);
  *D = dl_scratch(carve, terms, n, t, check);
  return 0;
}

// ---- the weighted sum in G2 ----------------------------------------------------------------------------------------------------------------------
// where a term's point comes from: 128 bytes each at pts, or — pts == nullptr — the registered table, term s reading key s below `wrap` and
// key s - wrap from there on (the check's two segments: the first t keys, then all n)
struct G2Src { const uint8_t* pts; const int32_t* key_xy; const uint8_t* key_inf; size_t wrap; };
// one lane per term.  No early return past the stop byte: the ladder's additions vote across the wave; a lane past the end walks the identity
// (bn254_dealing.h: g2msm_term).  skip: a device byte, non-zero = a kernel in front has settled the call already (wave-uniform: every lane leaves)
KERNEL void k_g2msm_term(G2Src src, const uint8_t* scalars, size_t m, int reduce, const uint8_t* skip, G2Jac* terms, uint8_t* term_st) {
  if (skip && *skip) return;
  const size_t s = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = s < m;
  const size_t at = live ? s : 0;
  G2Jac t;
  uint8_t st = ST_OK;
  if (src.pts) {
    g2msm_term(t, st, src.pts + 128 * at, scalars + 32 * at, reduce != 0, live);
  } else {
    const size_t key = at < src.wrap ? at : at - src.wrap;
    g2msm_term_key(t, src.key_xy + key * 4 * BN_LIMBS, src.key_inf[key] != 0, scalars + 32 * at, live);
  }
  if (!live) return;
  terms[s] = t;
  term_st[s] = st;
}
// lane per segment, the segments below wave_min terms (and the refused ones, which have none); wave per segment, the others — k_msm_sum_lane
// and k_msm_sum_wave over G2Jac, 128 bytes out.  A masked segment (gate) is left alone.
KERNEL void k_g2msm_sum_lane(const G2Jac* terms, const uint8_t* term_st, const uint64_t* seg, uint64_t m, const uint8_t* gate, size_t n, uint64_t wave_min,
                             uint8_t* out, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  uint8_t seg_st = MSM_SEG_MASKED;
  uint64_t len = live ? msm_seg_len(seg, i, m, gate, seg_st) : 0;
  const bool mine = live && seg_st != MSM_SEG_MASKED && (seg_st != ST_OK || len < wave_min);
  if (!mine) len = 0;
  if (!BN_WAVE_ANY(mine)) return;
  G2Jac acc;
  uint8_t st = ST_OK;
  msm_lane_sum(acc, st, terms, term_st, len ? seg[i] : 0, len);
  if (mine && seg_st != ST_OK) st = seg_st;
  G2Affine r;
  jac_to_affine(r, acc);
  if (!mine) return;
  if (st != ST_OK) r.inf = true;
  encode_g2(out + 128 * i, r);
  status[i] = st;
}
// LDS per workgroup (one wave): 64 slots of 220 B (G2Jac + the pad word) = 14 080 B, 256 B of counts, 512 B of indices, 64 B of statuses =
// 14 912 B; one wave per SIMD (at two the tree's additions spilled 62 registers), so four workgroups share a CU's 160 KiB: 59 648 B
KERNEL void k_g2msm_sum_wave(const G2Jac* terms, const uint8_t* term_st, const uint64_t* seg, uint64_t m, const uint8_t* gate, size_t n, uint64_t wave_min,
                                   uint8_t* out, uint8_t* status) {
  __shared__ G2JacSlot part[BN_WAVE];
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
      g2msm_encode(out + 128 * i, part[0].v, st[0]);
      status[i] = st[0];
    }
    __syncthreads();
  }
}
// terms and sums of m terms in n segments, enqueued on s; D holds m terms.  marks: the check's profiling events 2 and 3 around the sums
static int launch_g2msm(bn254_ctx* c, hipStream_t s, const G2Src& src, const uint8_t* d_scalars, size_t m, const uint64_t* d_seg, const uint8_t* d_gate, size_t n,
                        int reduce, const uint8_t* d_skip, const DlScratch& D, uint8_t* d_out, uint8_t* d_status, bool marks) {
  if (m) {
    k_g2msm_term<<<grid_for(m), BN_WAVE, 0, s>>>(src, d_scalars, m, reduce, d_skip, D.terms, D.term_st);
    HIP_TRY(hipGetLastError());
  }
  if (marks) PROF_MARK(2);
  const uint64_t wave_min = (uint64_t)c->collect_wave_min;
  k_g2msm_sum_lane<<<grid_for(n), BN_WAVE, 0, s>>>(D.terms, D.term_st, d_seg, (uint64_t)m, d_gate, n, wave_min, d_out, d_status);
  HIP_TRY(hipGetLastError());
  k_g2msm_sum_wave<<<(unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS), BN_WAVE, 0, s>>>(D.terms, D.term_st, d_seg, (uint64_t)m, d_gate, n, wave_min, d_out,
                                                                                                 d_status);
  HIP_TRY(hipGetLastError());
  if (marks) PROF_MARK(3);
  return 0;
}
// the sums alone, over terms another unit has written (bn254_host.h; bn254_reshare.hip: its terms are column-major over decoded points)
int launch_g2msm_sums(bn254_ctx* c, hipStream_t s, const G2Jac* terms, const uint8_t* term_st, size_t m, const uint64_t* d_seg, const uint8_t* d_gate, size_t n,
                      uint8_t* d_out, uint8_t* d_status) {
  const uint64_t wave_min = (uint64_t)c->collect_wave_min;
  k_g2msm_sum_lane<<<grid_for(n), BN_WAVE, 0, s>>>(terms, term_st, d_seg, (uint64_t)m, d_gate, n, wave_min, d_out, d_status);
  HIP_TRY(hipGetLastError());
  k_g2msm_sum_wave<<<(unsigned)(n < CL_WAVE_MAX_BLOCKS ? n : CL_WAVE_MAX_BLOCKS), BN_WAVE, 0, s>>>(terms, term_st, d_seg, (uint64_t)m, d_gate, n, wave_min, d_out,
                                                                                                 d_status);
  HIP_TRY(hipGetLastError());
  return 0;
}
// the _device form behind its argument checks, the number of terms known
static int g2msm_device(bn254_ctx* c, const uint8_t* d_points, const uint8_t* d_scalars, const uint64_t* d_seg, size_t m, size_t n, int reduce, uint8_t* d_out,
                        uint8_t* d_status, hipStream_t s) {
  if (m > 0xFFFFFFFFu || (m && (!d_points || !d_scalars))) return BN254_E_BAD_ARGUMENT;
  DlScratch D;
  if (const int rc = dl_scratch_reserve(c, m, 0, 0, false, &D)) return rc;
  CallDone call_done(c, s);
  const G2Src src = {d_points, nullptr, nullptr, 0};
  return launch_g2msm(c, s, src, d_scalars, m, d_seg, nullptr, n, reduce, nullptr, D, d_out, d_status, false);
}

// ---- the check of a dealing ------------------------------------------------------------------------------------------------------------------------
// one wave: the lowest key with a non-zero registration status; it (or t_over, the host's threshold > n) raises the stop byte and masks both
// segments, whose offsets {0, t, t + n_check} lane 0 writes too
KERNEL_SMALL void k_dl_scan(const uint8_t* key_st, uint32_t n, uint32_t t, uint32_t n_check, int t_over, uint32_t* bad_key, uint8_t* bad_st, uint8_t* skip,
                            uint8_t* gate, uint64_t* seg) {
  __shared__ uint32_t key[BN_WAVE];
  __shared__ uint8_t st[BN_WAVE];
  const unsigned l = threadIdx.x;
  dl_scan_lane(key[l], st[l], key_st, n, l);
  __syncthreads();
  if (l != 0) return;
  uint32_t k = key[0];
  uint8_t s = st[0];
  for (unsigned o = 1; o < BN_WAVE; ++o) dl_scan_fold(k, s, key[o], st[o]);
  *bad_key = k;
  *bad_st = s;
  const uint8_t stop = (k != UINT32_MAX || t_over) ? MSM_SEG_MASKED : 0;
  *skip = stop;
  gate[0] = gate[1] = stop;
  seg[0] = 0, seg[1] = t, seg[2] = (uint64_t)t + n_check;
}
// one wave: fact[0 .. n1) by a chunked product scan (bn254_dealing.h: dl_fact_*)
KERNEL_SMALL void k_dl_fact(Fr* fact, uint32_t n1, const uint8_t* skip) {
  __shared__ Fr part[BN_WAVE];
  if (skip && *skip) return;
  const unsigned l = threadIdx.x;
  part[l] = dl_fact_partial(n1, l);
  __syncthreads();
  if (l == 0) dl_fact_prefix(part);
  __syncthreads();
  dl_fact_write(fact, n1, l, part[l]);
}
// lane per table entry m in [0, n]; lane per key k < t: lambda_k to scalars[k], c_k to scalars[t + k] (c_j, j >= t, are the tables' pass's)
KERNEL_SMALL void k_dl_tables(Fr* inv, Fr* w, uint8_t* scalars, const Fr* fact, RandSeed seed, uint32_t n, uint32_t t, const uint8_t* skip) {
  if (skip && *skip) return;
  const size_t m = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (m > n) return;
  dl_tables(inv, w, scalars + 32 * (size_t)t, fact, seed.w, n, t, (uint32_t)m);
}
KERNEL_SMALL void k_dl_coeff(const Fr* fact, const Fr* inv, const Fr* w, uint32_t n, uint32_t t, uint8_t* scalars, const uint8_t* skip) {
  if (skip && *skip) return;
  const size_t k = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (k >= t) return;
  Fr lambda, ck;
  dl_coeff(lambda, ck, fact, inv, w, n, t, (uint32_t)k);
  fr_to_be(scalars + 32 * k, lambda);
  fr_to_be(scalars + 32 * ((size_t)t + k), ck);
}
KERNEL_SMALL void k_dl_settle(const uint32_t* bad_key, const uint8_t* bad_st, int t_over, const uint8_t* sums, const uint8_t* sum_st, DlResult* result) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  DlResult r;
  dl_settle(r, *bad_key, *bad_st, t_over != 0, sums, sum_st);
  *result = r;
}
// the three coefficient kernels for n keys and threshold t <= n, enqueued on s: D.scalars = lambda_0 .. lambda_t-1, c_0 .. c_n-1
static int launch_dl_coefficients(hipStream_t s, const DlScratch& D, const RandSeed& seed, uint32_t n, uint32_t t, const uint8_t* d_skip) {
  k_dl_fact<<<1, BN_WAVE, 0, s>>>(D.fact, n + 1, d_skip);
  HIP_TRY(hipGetLastError());
  k_dl_tables<<<grid_for((size_t)n + 1), BN_WAVE, 0, s>>>(D.inv, D.w, D.scalars, D.fact, seed, n, t, d_skip);
  HIP_TRY(hipGetLastError());
  k_dl_coeff<<<grid_for(t), BN_WAVE, 0, s>>>(D.fact, D.inv, D.w, n, t, D.scalars, d_skip);
  HIP_TRY(hipGetLastError());
  return 0;
}
// the largest key set the tables are sized for: n + 1 entries and t + n terms stay below 2^32
#define DL_MAX_KEYS 0x7FFFFFFFu

extern "C" {

int bn254_batch_g2_msm_device(bn254_ctx* c, const uint8_t* d_points, const uint8_t* d_scalars, const uint64_t* d_seg_off, size_t n, int reduce_scalar,
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
  return g2msm_device(c, d_points, d_scalars, d_seg_off, (size_t)m, n, reduce_scalar, d_out, d_status, s);
}
int bn254_batch_g2_msm(bn254_ctx* c, const uint8_t* points, const uint8_t* scalars, const uint64_t* seg_off, size_t n, int reduce_scalar, uint8_t* out,
                       uint8_t* status) {
  if (!c || n > 0xFFFFFFFFu || (n && (!seg_off || !out || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!offsets_ok(seg_off, n)) return BN254_E_BAD_ARGUMENT;
  const size_t total = (size_t)seg_off[n];
  if (total && (!points || !scalars)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_points = st.in(0, points, total * 128), *d_scalars = st.in(1, scalars, total * 32), *d_seg = st.in(2, seg_off, (n + 1) * sizeof(uint64_t));
  uint8_t *d_out = st.out(3, n * 128, out), *d_status = st.out(4, n, status);
  if (st.ok()) st.rc = g2msm_device(c, d_points, d_scalars, (const uint64_t*)d_seg, total, n, reduce_scalar, d_out, d_status, c->stream);
  return st.finish();
}

// host-synchronous, like a registration: the context is quiesced first, the outputs are written when the call returns
int bn254_ctx_check_dealing(bn254_ctx* c, uint32_t threshold, const uint8_t* seed32, uint32_t flags, uint8_t* group_pk, uint8_t* status, uint32_t* bad_key) {
  if (!c || threshold == 0 || flags != 0 || !seed32 || !group_pk || !status || c->n_keys == 0 || c->n_keys > DL_MAX_KEYS) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  const uint32_t n = (uint32_t)c->n_keys, t = threshold;
  const bool t_over = t > n;
  // t == n: nothing to check — the second segment is empty, its sum the identity
  const uint32_t n_check = (!t_over && t < n) ? n : 0;
  const size_t m = t_over ? 0 : (size_t)t + n_check;
  DlScratch D;
  if (const int rc = dl_scratch_reserve(c, m, n, t_over ? n : t, true, &D)) return rc;
  hipStream_t s = c->stream;
  DlResult home;
  HostStaging st(c);
  st.copy_back(&home, D.result, offsetof(DlResult, status) + 1);
  if (!st.ok()) return st.rc;
  // ms[0] = the key scan and the coefficients, ms[1] = the terms, ms[2] = the sums, ms[3] = the verdict
  PROF_MARK(0);
  k_dl_scan<<<1, BN_WAVE, 0, s>>>(c->key_st, n, t_over ? 0 : t, n_check, t_over ? 1 : 0, D.bad_key, D.bad_st, D.skip, D.gate, D.seg);
  HIP_TRY(hipGetLastError());
  if (!t_over) {
    if (const int rc = launch_dl_coefficients(s, D, rand_seed_from(seed32), n, t, D.skip)) return rc;
    PROF_MARK(1);
    const G2Src src = {nullptr, c->key_xy, c->key_inf, t};
    if (const int rc = launch_g2msm(c, s, src, D.scalars, m, D.seg, D.gate, 2, 0, D.skip, D, D.sums, D.sum_st, true)) return rc;
  } else {
    PROF_MARK(1);
    PROF_MARK(2);
    PROF_MARK(3);
  }
  k_dl_settle<<<1, BN_WAVE, 0, s>>>(D.bad_key, D.bad_st, t_over ? 1 : 0, D.sums, D.sum_st, D.result);
  HIP_TRY(hipGetLastError());
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  if (const int rc = st.finish()) return rc;
  memcpy(group_pk, home.pk, 128);
  *status = home.status;
  if (bad_key) *bad_key = home.bad_key;
  return 0;
}

int bn254_debug_dealing_coefficients(bn254_ctx* c, size_t n_keys, uint32_t threshold, const uint8_t* seed32, uint8_t* out) {
  if (!c || n_keys == 0 || n_keys > DL_MAX_KEYS || threshold == 0 || threshold > n_keys || !seed32 || !out) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t n = (uint32_t)n_keys, t = threshold;
  DlScratch D;
  if (const int rc = dl_scratch_reserve(c, 0, n, t, true, &D)) return rc;
  HostStaging st(c);
  st.copy_back(out, D.scalars + 32 * (size_t)t, 32 * (size_t)n);
  if (!st.ok()) return st.rc;
  if (const int rc = launch_dl_coefficients(c->stream, D, rand_seed_from(seed32), n, t, nullptr)) return rc;
  return st.finish();
}

}  // extern "C"
