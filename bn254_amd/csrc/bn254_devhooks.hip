// Translation unit of libbn254hip.so: DEVELOPER HOOKS — the element-wise test entry points the parity tests compare layer by layer with the
// oracle (bn254_debug_*) and the measurement entry points behind bench.py's roofline figures (bn254_probe_*).  Not part of the drop-in ABI
// (include/bn254_hip.h, section BN254_DEV_HOOKS): no reference function corresponds to any of them.
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
#include "bn254_fq2_hook.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"

// --- test hooks ---------------------------------------------------------------------------
KERNEL_SMALL void k_debug_fp_op(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out, uint8_t* status) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  uint32_t any = 0;
  Fp x, y, r;
  bool ok = fp_from_be(x, a + 32 * i, any);
  if (b) ok = fp_from_be(y, b + 32 * i, any) && ok; else y = fp_zero();
  uint8_t st = ok ? ST_OK : ST_NOT_MEMBER;
  switch (op) {
    case 0: r = fp_mul(x, y); break;
    case 1: r = fp_add(x, y); break;
    case 2: r = fp_sub(x, y); break;
    case 3: r = fp_inv(x); break;
    case 4: r = fp_sqr(x); break;
    default: if (!fp_sqrt(r, x) && st == ST_OK) st = ST_NOT_MEMBER; break;
  }
  fp_to_be(out + 32 * i, r);
  status[i] = st;
}
// The try loop's treatment of ONE chosen digest value (32 B big-endian): range rules + mod_u256, the Jacobi filter of
// k_hash_round and the square root of k_hash_finish.  status 0 = yields the point written to out, 1 = next counter;
// bit 7 set = filter and square root disagree (never expected).
KERNEL_SMALL void k_debug_hash_candidate(const uint8_t* h, size_t n, uint8_t* out, uint8_t* status) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  U256 x;
  const uint32_t* w = (const uint32_t*)(h + 32 * i);
#pragma unroll
  for (int k = 0; k < 8; ++k) x.w[7 - k] = __builtin_bswap32(w[k]);
  bool cand = hash_reduce_candidate(x);
  bool filt = false, ok = false;
  G1Affine p;
  g1_set_generator(p);
  if (cand) {
    Fp xm, rhs;
    hash_curve_rhs(xm, rhs, x);
    filt = u256_is_square_mod_q(fp_to_u256(rhs));
    ok = hash_point_from_candidate(p, x);
  }
  if (!ok) p.inf = true;
  encode_g1(out + 64 * i, p);
  status[i] = (uint8_t)((ok ? 0 : 1) | (filt != ok ? 0x80 : 0));
}
// The Jacobi symbol of the hash filter, one value per lane (include/bn254_hip.h: bn254_debug_jacobi).  mode 0: a < q straight into
// u256_is_square_mod_q | 1: a = a candidate x < q through hash_curve_rhs and fp_to_u256 as hash_try_filter does, bit 1 = the square root's
// answer | 2: the symbol (a / b) through the same passes (u256_jacobi_symbol).  value = what the passes were handed; bit 7 = operand refused.
__device__ __forceinline__ U256 u256_from_be(const uint8_t* p) {
  U256 x;
  const uint32_t* w = (const uint32_t*)p;
#pragma unroll
  for (int k = 0; k < 8; ++k) x.w[7 - k] = __builtin_bswap32(w[k]);
  return x;
}
KERNEL_SMALL void k_debug_jacobi(int mode, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* value, uint8_t* flags) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const U256 x = u256_from_be(a + 32 * i);
  U256 v = x;
  uint8_t fl = 0;
  if (mode == 2) {
    const U256 m = u256_from_be(b + 32 * i);
    uint32_t above = m.w[0] & ~1u;                     // an odd m is >= 3 iff it has a bit above bit 0
#pragma unroll
    for (int k = 1; k < 8; ++k) above |= m.w[k];
    const bool ok = (m.w[0] & 1u) && above != 0 && !u256_geq(x.w, m.w);
    if (ok) fl = (uint8_t)u256_jacobi_symbol(x, m); else fl = 0x80;
  } else if (u256_geq(x.w, C_Q)) {
    fl = 0x80;
  } else if (mode == 1) {
    Fp xm, rhs;
    hash_curve_rhs(xm, rhs, x);
    v = fp_to_u256(rhs);
    G1Affine p;
    fl = (uint8_t)((u256_is_square_mod_q(v) ? 1 : 0) | (hash_point_from_candidate(p, x) ? 2 : 0));
  } else {
    fl = u256_is_square_mod_q(x) ? 1 : 0;
  }
  if (fl & 0x80) { for (int k = 0; k < 8; ++k) v.w[k] = 0; }
  uint32_t* o = (uint32_t*)(value + 32 * i);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = __builtin_bswap32(v.w[7 - k]);
  flags[i] = fl;
}
// One Fq2 primitive per lane on raw limb vectors, through the classic fp2_* / fp_* of bn254_field.h (bn254_fq2_hook.h holds the one switch all four
// builds share; the pair layout's kernel is k_debug_fq2_limbs_pair in bn254_pair.hip).  in: n x 4 operands x 18 limbs, coef: n x 4.
KERNEL_SMALL void k_debug_fq2_limbs(int op, const int32_t* in, const int32_t* coef, size_t n, int32_t* out, uint8_t* flags) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const int32_t* p = in + i * (BN_FQ2_HOOK_OPERANDS * BN_FQ2_HOOK_WORDS);
  const Fp2 a = fq2_hook_load(p, 0), b = fq2_hook_load(p + BN_FQ2_HOOK_WORDS, 0), c = fq2_hook_load(p + 2 * BN_FQ2_HOOK_WORDS, 0),
            d = fq2_hook_load(p + 3 * BN_FQ2_HOOK_WORDS, 0);
  int32_t k[BN_FQ2_HOOK_OPERANDS];
#pragma unroll
  for (int t = 0; t < BN_FQ2_HOOK_OPERANDS; ++t) k[t] = coef[i * BN_FQ2_HOOK_OPERANDS + t];
  bool flag;
  const Fp2 r = fq2_hook_op(op, a, b, c, d, b.c0, k, flag);
  int32_t* o = out + i * BN_FQ2_HOOK_WORDS;
#pragma unroll
  for (int j = 0; j < BN_LIMBS; ++j) { o[j] = r.c0.v[j]; o[BN_LIMBS + j] = r.c1.v[j]; }
  flags[i] = flag ? 1 : 0;
}
__device__ __forceinline__ void decode_fp12(Fp12& f, const uint8_t* b) {
  uint32_t any = 0;
  Fp2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int k = 0; k < 6; ++k) { fp_from_be(c[k]->c0, b + 64 * k, any); fp_from_be(c[k]->c1, b + 64 * k + 32, any); }
}
KERNEL void k_debug_fp12_op(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  Fp12 x, y, r;
  decode_fp12(x, a + 384 * i);
  if (b) decode_fp12(y, b + 384 * i); else fp12_set_one(y);
  switch (op) {
    case 0: fp12_mul(r, x, y); break;
    case 1: fp12_sqr(r, x); break;
    case 2: fp12_inv(r, x); break;
    case 3: fp12_conj(r, x); break;
    case 4: fp12_frob(r, x, 1); break;
    case 5: fp12_frob(r, x, 2); break;
    case 6: fp12_frob(r, x, 3); break;
    case 7: fp12_cyclotomic_sqr(r, x); break;
    default: { Fp12 acc; final_exponentiation(r, x, acc); } break;
  }
  encode_fp12(out + 384 * i, r);
}

// test hook: LIMB vectors straight into the F planes of the workspace (12 coefficients x 9 int32 limbs per item, Gt order) — the input of a
// final exponentiation with non-canonical / extreme-digit representatives that no byte decoder would produce
KERNEL_SMALL void k_debug_load_f(const int32_t* limbs, size_t n, Ws ws) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  for (int e = 0; e < 12; ++e) {
    Fp x;
#pragma unroll
    for (int k = 0; k < BN_LIMBS; ++k) x.v[k] = limbs[(i * 12 + e) * BN_LIMBS + k];
    ws_store_fp(ws, PL_F0 + e, i, x);
  }
  ws_byte(ws, BY_ST_DECODE, i) = ST_OK;
  ws_byte(ws, BY_ST_HASH, i) = ST_OK;
}
// test hook: n affine G1 points of the P1 planes from `base` as 64-byte encodings (the identity: zeros)
KERNEL_SMALL void k_debug_read_p1(Ws ws, size_t base, size_t n, uint8_t* out) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G1Affine p;
  ws_load_g1(ws, PL_P1X, BY_P1_INF, base + i, p);
  encode_g1(out + 64 * i, p);
}

// Fr, element-wise (bn254_fr.h): operands as 32 big-endian bytes, reduced on load.  op 0 mul, 1 add, 2 sub, 3 neg, 4 inv (0 -> 0),
// 5 the round trip into Montgomery form and back, 6 the low 32 bits of a (its last four bytes) loaded as a uint32_t
KERNEL_SMALL void k_debug_fr_op(int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const Fr x = fr_from_be(a + 32 * i), y = b ? fr_from_be(b + 32 * i) : fr_zero();
  Fr r;
  switch (op) {
    case 0: r = fr_mul(x, y); break;
    case 1: r = fr_add(x, y); break;
    case 2: r = fr_sub(x, y); break;
    case 3: r = fr_neg(x); break;
    case 4: r = fr_inv(x); break;
    case 6: r = fr_from_u32(__builtin_bswap32(((const uint32_t*)(a + 32 * i))[7])); break;
    default: r = x; break;
  }
  fr_to_be(out + 32 * i, r);
}
// the Lagrange coefficient at zero of every point within its segment (bn254_threshold.h: th_lagrange_points): one lane per point, which
// finds its segment by a search of the (host-checked, non-decreasing) offsets
KERNEL_SMALL void k_debug_lagrange(const uint32_t* x, const uint64_t* seg, size_t m, size_t n, uint8_t* out) {
  size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j >= m) return;
  size_t a = 0, b = n;                                 // the first segment that ends behind j
  while (a < b) {
    const size_t mid = (a + b) >> 1;
    if (seg[mid + 1] > j) b = mid; else a = mid + 1;
  }
  const uint64_t lo = seg[a], len = seg[a + 1] - lo;
  fr_to_be(out + 32 * j, th_lagrange_points(x + lo, len, j - lo));
}

// ---- in-process issue-rate probe (bench.py's roofline calibration) --------------------------------------------
// 16 independent chains of one instruction, 4096 trips, on every SIMD of the device with `waves_per_simd` waves each
// (256-thread workgroups = one wave per SIMD of a CU, like the pair kernels).  op 0: v_mad_u64_u32, 1: v_add_u32,
// 2: v_mul_lo_u32.  The standalone sweep over more instructions is bn254_amd/csrc/microbench/valu_rates.hip.
#define PROBE_ITERS 4096
#define PROBE_CHAINS 16
template <int OP>
__global__ void __launch_bounds__(256) k_issue_probe(uint32_t* out, uint32_t seed, unsigned long long* clk) {
  unsigned long long clk0 = 0, wall0 = 0;
  if (clk && threadIdx.x == 0) { clk0 = clock64(); wall0 = wall_clock64(); }
  uint32_t a = seed + threadIdx.x * 2654435761u, b = seed ^ (threadIdx.x * 40503u + 977u);
  uint64_t acc[PROBE_CHAINS];
#pragma unroll
  for (int j = 0; j < PROBE_CHAINS; ++j) acc[j] = a + j;
  for (int i = 0; i < PROBE_ITERS; ++i) {
#pragma unroll
    for (int j = 0; j < PROBE_CHAINS; ++j) {
      if (OP == 0) {
        asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[j]) : "v"(a), "v"(b) : "vcc");
      } else if (OP == 1) {
        uint32_t lo = (uint32_t)acc[j];
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(lo) : "v"(a));
        acc[j] = lo;
      } else {
        uint32_t lo = (uint32_t)acc[j];
        asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(lo) : "v"(b));
        acc[j] = lo;
      }
    }
  }
  uint64_t sum = 0;
#pragma unroll
  for (int j = 0; j < PROBE_CHAINS; ++j) sum += acc[j];
  out[(size_t)blockIdx.x * 256 + threadIdx.x] = (uint32_t)sum ^ (uint32_t)(sum >> 32);
  if (clk && threadIdx.x == 0 && blockIdx.x < BN_CLK_MAX_WG) {     // slot 2 of the clock probe (bn254_ws.h): this kernel's own clock
    unsigned long long* p = clk + ((size_t)2 * BN_CLK_MAX_WG + blockIdx.x) * 2;
    p[0] += clock64() - clk0; p[1] += wall_clock64() - wall0;
  }
}
// test hook: entries first .. first + n - 1 of a pool / table of the aggregate verify as canonical bytes (zeros under the identity flag) and
// their raw status bytes.  The words are read under the stored-word contract of bn254_pooltab.h (|value| <= q), which fp_to_be accepts.
KERNEL_SMALL void k_debug_read_pool(Pool pool, size_t first, size_t n, uint8_t* out, uint8_t* flags) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const size_t j = first + i;
  const uint8_t st = pool.st[j];
  if (pool.g2) {
    G2Affine q;
    q.x.c0 = pool_load_fp(pool, 0, j); q.x.c1 = pool_load_fp(pool, 1, j); q.y.c0 = pool_load_fp(pool, 2, j); q.y.c1 = pool_load_fp(pool, 3, j);
    q.inf = (st & 0x80) != 0;
    encode_g2(out + 128 * i, q);
  } else {
    G1Affine p;
    p.x = pool_load_fp(pool, 0, j); p.y = pool_load_fp(pool, 1, j);
    p.inf = (st & 0x80) != 0;
    encode_g1(out + 64 * i, p);
  }
  flags[i] = st;
}

extern "C" {

// the tables of the registered pools as they stand on the device (include/bn254_hip.h); which = -1: the query form
int bn254_debug_agg_tables(bn254_ctx* c, int which, size_t first, size_t count, uint8_t* points, uint8_t* flags) {
  if (!c || which < -1 || which > 7 || !points) return BN254_E_BAD_ARGUMENT;
  const AggTables& t = c->reg_pools;
  if (!t.valid) return BN254_E_BAD_ARGUMENT;          // nothing registered, or a call with raw pools has overwritten the buffers since
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  if (which < 0) {
    const uint64_t q[5] = {(uint64_t)t.n_groups, (uint64_t)t.groups4, (uint64_t)t.wide2, (uint64_t)t.wide1, (uint64_t)t.t4_builder};
    memcpy(points, q, sizeof q);
    return 0;
  }
  if (!flags) return BN254_E_BAD_ARGUMENT;
  // entries of each table; 0 = not built for this registration (the buffer may still hold an older registration's table)
  const size_t entries[8] = {t.n_signers, t.n_msgs * t.n_signers, t.n_msgs, t.n_groups * 256, t.n_msgs * t.groups4 * 16,
                             t.wide2 ? ((t.n_groups + 1) / 2) * 65536 : 0, t.wide1 ? t.n_msgs * t.n_groups * 256 : 0,
                             t.t4_builder == 1 ? t.n_msgs * 2 * t.groups4 * 4 : 0};
  const size_t total = entries[which];
  const Pool& p = c->pool[which];
  if (total == 0 || !p.planes || total > p.stride) return BN254_E_BAD_ARGUMENT;
  if (first > total || count > total - first) return BN254_E_BAD_ARGUMENT;
  if (count == 0) return 0;
  const size_t sz = p.g2 ? 128 : 64;
  HostStaging st(c);
  uint8_t *d_out = st.out(0, count * sz, points), *d_flags = st.out(1, count, flags);
  if (!st.ok()) return st.rc;
  k_debug_read_pool<<<grid_for(count), BN_WAVE, 0, c->stream>>>(p, first, count, d_out, d_flags);
  HIP_TRY(hipGetLastError());
  return st.finish();
}
// the routing table of the context (bn254_ws.h: bn_route_table) — tests iterate its boundaries
// what the key deduplication of the last bn254_batch_verify_device decided on the device (bn254_keydedup.hip): out = {ran, distinct keys D,
// flags (1 probe overflow, 2 degenerate line), items of the keyed Miller kernel, items of the generic one}; ran = 0: the call did not take
// the dedup at all (other route, option off, no room), the other words are then 0.  Synchronises the device.
int bn254_debug_key_dedup_last(bn254_ctx* c, uint32_t out[5]) {
  if (!c || !out) return BN254_E_BAD_ARGUMENT;
  for (int i = 0; i < 5; ++i) out[i] = 0;
  if (!c->kd_last_run || !c->kd_ctl) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out + 1, c->kd_ctl, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  out[0] = 1;
  return 0;
}
// what that call did with the key cache (BN254_OPT_KEY_CACHE; k_kd_match): out = {ran, distinct keys D, keys found in the cache, keys built,
// dropped (1 the misses did not fit the free rows, 2 the cache was emptied before the call: other flags or options, moved buffers, the
// option at 0)}; a call the thresholds refuse looks nothing up: hits = built = 0.  Synchronises the device.
int bn254_debug_key_cache_last(bn254_ctx* c, uint32_t out[5]) {
  if (!c || !out) return BN254_E_BAD_ARGUMENT;
  for (int i = 0; i < 5; ++i) out[i] = 0;
  if (!c->kd_last_run || !c->kd_ctl) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t ctl[KD_CTL_WORDS];
  HIP_TRY(hipMemcpy(ctl, c->kd_ctl, sizeof ctl, hipMemcpyDeviceToHost));
  out[0] = 1; out[1] = ctl[KD_CTL_D]; out[2] = ctl[KD_CTL_HITS]; out[3] = ctl[KD_CTL_BUILD]; out[4] = ctl[KD_CTL_DROPPED];
  return 0;
}
// the line tables as they stand on the device: which = 0 the tables of the keys of the last key dedup (key ids as k_kd_insert gave them; rep = the
// item that represents each key; each key's table is read from the row the cache keeps it in; a call the thresholds refused has none:
// BN254_E_BAD_ARGUMENT, nothing written), 1 the registered tables of
// bn254_ctx_register_keys (rep is not written)
int bn254_debug_key_tables(bn254_ctx* c, int which, size_t first, size_t count, int32_t* lines, uint32_t* rep, uint8_t* st, uint8_t* inf) {
  if (!c || !lines || (which != 0 && which != 1)) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t per_key = (size_t)BN_N_FIXED_LINES * BN_KEY_LINE_WORDS;
  const int32_t* src;
  const uint8_t *src_st, *src_inf;
  if (which == 0) {
    uint32_t ctl[KD_CTL_WORDS];
    if (!c->kd_last_run || !c->kd_ctl || !c->kd_lines_last) return BN254_E_BAD_ARGUMENT;
    HIP_TRY(hipMemcpy(ctl, c->kd_ctl, sizeof ctl, hipMemcpyDeviceToHost));
    if (first + count > ctl[KD_CTL_D] || first + count > c->kd_keys_cap) return BN254_E_BAD_ARGUMENT;
    if (ctl[KD_CTL_BUILD] + ctl[KD_CTL_HITS] != ctl[KD_CTL_D]) return BN254_E_BAD_ARGUMENT;   // a call the thresholds refused: it has no tables (nothing written)
    if (rep) HIP_TRY(hipMemcpy(rep, c->kd_rep_last + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    // rows, statuses and identity flags in one host block: [count] u32 | [kd_keys_cap] st | [kd_keys_cap] inf
    const size_t cap = c->kd_keys_cap;
    uint8_t* h = (uint8_t*)malloc(count * sizeof(uint32_t) + 2 * cap + 1);
    if (!h) return BN254_E_NO_MEMORY;
    const uint32_t* rows = (const uint32_t*)h;
    uint8_t *h_st = h + count * sizeof(uint32_t), *h_inf = h_st + cap;
    hipError_t e = count ? hipMemcpy(h, c->kd_row_of_last + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(h_st, c->kd_st_last, cap, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_inf, c->kd_inf_last, cap, hipMemcpyDeviceToHost);
    int rc = e == hipSuccess ? 0 : -(int)e;
    for (size_t k = 0; k < count && !rc; ++k) {
      const size_t r = rows[k];
      if (r >= cap) { rc = BN254_E_BAD_ARGUMENT; break; }
      e = hipMemcpy(lines + k * per_key, c->kd_lines_last + r * per_key, per_key * sizeof(int32_t), hipMemcpyDeviceToHost);
      if (e != hipSuccess) rc = -(int)e;
      if (st) st[k] = h_st[r];
      if (inf) inf[k] = h_inf[r];
    }
    free(h);
    return rc;
  } else {
    if (!c->key_lines || first + count > c->n_keys) return BN254_E_BAD_ARGUMENT;
    src = c->key_lines; src_st = c->key_st; src_inf = c->key_inf;
  }
  HIP_TRY(hipMemcpy(lines, src + first * per_key, count * per_key * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (st) HIP_TRY(hipMemcpy(st, src_st + first, count, hipMemcpyDeviceToHost));
  if (inf) HIP_TRY(hipMemcpy(inf, src_inf + first, count, hipMemcpyDeviceToHost));
  return 0;
}
// the folded rows (kd.fold) of the keys of the last key dedup, in the order and under the conditions of bn254_debug_key_tables(which = 0)
int bn254_debug_key_fold_tables(bn254_ctx* c, size_t first, size_t count, int32_t* rows_out) {
  if (!c || !rows_out) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t per_key = (size_t)BN_N_FOLD_ROWS * BN_KEY_FOLD_WORDS;
  uint32_t ctl[KD_CTL_WORDS];
  if (!c->kd_last_run || !c->kd_ctl || !c->kd_fold_last) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipMemcpy(ctl, c->kd_ctl, sizeof ctl, hipMemcpyDeviceToHost));
  if (first + count > ctl[KD_CTL_D] || first + count > c->kd_keys_cap) return BN254_E_BAD_ARGUMENT;
  if (ctl[KD_CTL_BUILD] + ctl[KD_CTL_HITS] != ctl[KD_CTL_D]) return BN254_E_BAD_ARGUMENT;   // a call the thresholds refused: it has no tables
  if (count == 0) return 0;
  uint32_t* rows = (uint32_t*)malloc(count * sizeof(uint32_t));
  if (!rows) return BN254_E_NO_MEMORY;
  hipError_t e = hipMemcpy(rows, c->kd_row_of_last + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost);
  int rc = e == hipSuccess ? 0 : -(int)e;
  for (size_t k = 0; k < count && !rc; ++k) {
    if (rows[k] >= c->kd_keys_cap) { rc = BN254_E_BAD_ARGUMENT; break; }
    e = hipMemcpy(rows_out + k * per_key, c->kd_fold_last + (size_t)rows[k] * per_key, per_key * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = -(int)e;
  }
  free(rows);
  return rc;
}
static int debug_rand_last(bn254_ctx* c, int ran, const uint32_t* stats, uint64_t out[6]) {
  if (!c || !out) return BN254_E_BAD_ARGUMENT;
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (!ran || !stats) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t st[5];
  HIP_TRY(hipMemcpy(st, stats, sizeof st, hipMemcpyDeviceToHost));
  out[0] = 1;
  for (int i = 0; i < 5; ++i) out[i + 1] = st[i];
  return 0;
}
int bn254_debug_agg_rand_last(bn254_ctx* c, uint64_t out[6]) { return debug_rand_last(c, c ? c->aggr_last_ran : 0, c ? c->aggr_stats : nullptr, out); }
int bn254_debug_bitmap_rand_last(bn254_ctx* c, uint64_t out[6]) { return debug_rand_last(c, c ? c->bmr_last_ran : 0, c ? c->bmr_stats : nullptr, out); }
// bn254_batch_collect_keyed_bitmap_randomized: what the slices of the last call did, summed on the device by the call itself
int bn254_debug_collect_rand_last(bn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BN254_E_BAD_ARGUMENT;
  for (int i = 0; i < 4; ++i) out[i] = 0;
  if (!c->clr_last_ran || !c->clr_stats) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t st[4];
  HIP_TRY(hipMemcpy(st, c->clr_stats, sizeof st, hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; ++i) out[i] = st[i];
  return 0;
}
// bn254_batch_collect_keyed_bitmap_optimistic: what the last call did, summed on the device by the call itself
int bn254_debug_collect_opt_last(bn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BN254_E_BAD_ARGUMENT;
  for (int i = 0; i < 4; ++i) out[i] = 0;
  if (!c->clo_last_ran || !c->clo_stats) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t st[4];
  HIP_TRY(hipMemcpy(st, c->clo_stats, sizeof st, hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; ++i) out[i] = st[i];
  return 0;
}
// bn254_batch_threshold_combine_keyed_optimistic: {tuples checked, passed, sent the exact way, shares verified exactly} of its last call
int bn254_debug_threshold_opt_last(bn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BN254_E_BAD_ARGUMENT;
  for (int i = 0; i < 4; ++i) out[i] = 0;
  if (!c->tho_last_ran || !c->tho_stats) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t st[4];
  HIP_TRY(hipMemcpy(st, c->tho_stats, sizeof st, hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; ++i) out[i] = st[i];
  return 0;
}
// bn254_batch_merge_keyed_bitmap_optimistic: the same four of its last call, the fourth in partials
int bn254_debug_merge_opt_last(bn254_ctx* c, uint64_t out[4]) {
  if (!c || !out) return BN254_E_BAD_ARGUMENT;
  for (int i = 0; i < 4; ++i) out[i] = 0;
  if (!c->mgo_last_ran || !c->mgo_stats) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t st[4];
  HIP_TRY(hipMemcpy(st, c->mgo_stats, sizeof st, hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; ++i) out[i] = st[i];
  return 0;
}
// The groups of the last randomised call, read from where it left them (bn254_host.h: aggr_last): the call itself launches and copies
// nothing for this.  dims = {groups, table pairs}; with group_cap / pair_cap too small only dims is written.
static int debug_rand_sums(bn254_ctx* c, int ran, const AggrLast& L, uint64_t dims[2], size_t group_cap, size_t pair_cap, uint32_t* nagg, uint8_t* verdict,
                           uint8_t* s_g, uint64_t* first_pair, uint32_t* pair_key, uint8_t* pair_point) {
  if (!c || !dims) return BN254_E_BAD_ARGUMENT;
  dims[0] = dims[1] = 0;
  if (!ran) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t ng = L.ng, tbase = L.tbase;
  uint64_t end = 0;
  HIP_TRY(hipMemcpy(&end, L.ghi + (ng - 1), sizeof end, hipMemcpyDeviceToHost));
  const size_t n_tp = (size_t)(end - tbase);
  dims[0] = ng;
  dims[1] = n_tp;
  if (group_cap < ng || pair_cap < n_tp) return 0;
  if (!nagg || !verdict || !s_g || !first_pair || (n_tp && (!pair_key || !pair_point))) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipMemcpy(nagg, L.nagg, ng * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(verdict, L.gst, ng, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(first_pair, L.glo, ng * sizeof(uint64_t), hipMemcpyDeviceToHost));
  for (size_t g = 0; g < ng; ++g) first_pair[g] -= tbase;
  first_pair[ng] = n_tp;
  if (n_tp) HIP_TRY(hipMemcpy(pair_key, L.bkey + tbase, n_tp * sizeof(uint32_t), hipMemcpyDeviceToHost));
  int rc;
  if ((rc = stage_reserve(c, 0, 64 * (ng > n_tp ? ng : n_tp)))) return rc;
  k_debug_read_p1<<<grid_for(ng), BN_WAVE, 0, c->stream>>>(c->ws, L.cbase, ng, c->stage[0]);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(s_g, c->stage[0], 64 * ng, hipMemcpyDeviceToHost));
  if (n_tp) {
    k_debug_read_p1<<<grid_for(n_tp), BN_WAVE, 0, c->stream>>>(c->ws, tbase, n_tp, c->stage[0]);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(pair_point, c->stage[0], 64 * n_tp, hipMemcpyDeviceToHost));
  }
  return 0;
}
int bn254_debug_agg_rand_sums(bn254_ctx* c, uint64_t dims[2], size_t group_cap, size_t pair_cap, uint32_t* nagg, uint8_t* verdict, uint8_t* s_g,
                              uint64_t* first_pair, uint32_t* pair_key, uint8_t* pair_point) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  return debug_rand_sums(c, c->aggr_last_ran && c->aggr_buf, c->aggr_last, dims, group_cap, pair_cap, nagg, verdict, s_g, first_pair, pair_key, pair_point);
}
int bn254_debug_bitmap_rand_sums(bn254_ctx* c, uint64_t dims[2], size_t group_cap, size_t pair_cap, uint32_t* nagg, uint8_t* verdict, uint8_t* s_g,
                                 uint64_t* first_pair, uint32_t* pair_key, uint8_t* pair_point) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  return debug_rand_sums(c, c->bmr_last_ran && c->bmr_buf, c->bmr_last, dims, group_cap, pair_cap, nagg, verdict, s_g, first_pair, pair_key, pair_point);
}
int bn254_debug_route_table(bn254_ctx* c, uint64_t* max_n, int* miller, int* fe, int cap) {
  if (!c || !max_n || !miller || !fe || cap < 5) return BN254_E_BAD_ARGUMENT;
  size_t m[5];
  BnRoute r[5];
  const int rows = bn_route_table(route_limits(c), m, r, 5);
  for (int i = 0; i < rows; ++i) { max_n[i] = m[i] == (size_t)-1 ? UINT64_MAX : (uint64_t)m[i]; miller[i] = r[i].miller; fe[i] = r[i].fe; }
  return rows;
}

// issue-rate probe: wave-instructions per second of `op` with `waves_per_simd` waves on every SIMD, timed with HIP events
int bn254_probe_issue_rate(bn254_ctx* c, int op, int waves_per_simd, double* wave_inst_per_s, int* n_simd) {
  if (!c || !wave_inst_per_s || op < 0 || op > 2 || waves_per_simd < 1 || waves_per_simd > 8) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, c->device));
  const int n_cu = prop.multiProcessorCount, blocks = n_cu * waves_per_simd;
  int rc;
  if ((rc = stage_reserve(c, 0, sizeof(uint32_t) * 256 * (size_t)blocks))) return rc;
  uint32_t* out = (uint32_t*)c->stage[0];
  ScopedEvents ev;                                   // destroyed on every path out, the early error returns included
  HIP_TRY(ev.create());
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  float best = 0;
  for (int rep = 0; rep < 3; ++rep) {       // first repetition warms up; keep the fastest
    HIP_TRY(hipEventRecord(e0, c->stream));
    if (op == 0) k_issue_probe<0><<<blocks, 256, 0, c->stream>>>(out, 12345u, c->ws.clk);
    else if (op == 1) k_issue_probe<1><<<blocks, 256, 0, c->stream>>>(out, 12345u, c->ws.clk);
    else k_issue_probe<2><<<blocks, 256, 0, c->stream>>>(out, 12345u, c->ws.clk);
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (rep > 0 && (best == 0 || ms < best)) best = ms;
  }
  *wave_inst_per_s = (double)PROBE_ITERS * PROBE_CHAINS * 4.0 * blocks / (best * 1e-3);
  if (n_simd) *n_simd = n_cu * 4;
  return 0;
}

// Measurement: the product leaves of one verify's Miller loop alone (k_leaf_floor_pair, bn254_pair.hip) on the planes the last verify
// left in the workspace (n <= the size of that batch); ms = the kernel's duration (HIP events), best of 3 after a warm-up launch.
int bn254_probe_leaf_floor(bn254_ctx* c, size_t n, int mode, float* ms) {
  if (!c || !ms || n == 0 || n > c->ws.stride || mode < 0 || mode > 7) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  ScopedEvents ev;                                   // destroyed on every path out, the early error returns included
  HIP_TRY(ev.create());
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  float best = 0;
  int rc = 0;
  for (int rep = 0; rep < 4 && rc == 0; ++rep) {
    HIP_TRY(hipEventRecord(e0, c->stream));
    rc = bn254_pair_leaf_floor(n, c->ws, c->stream, mode);
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    if (rep > 0 && (best == 0 || t < best)) best = t;
  }
  *ms = best;
  return rc;
}

// Measurement: the final exponentiation's accumulator machine on a caller-supplied program (pairs of bytes (opcode, argument), ended by
// (0, 0); opcodes 1 LOAD s, 2 STORE s, 3 CSQR, 4 MUL s, 5 CONJ, 6 FROB k, 7 INV — bn254_pairing.h) for n lane pairs, on whatever the
// F planes of the workspace hold (run a verify first).  ms = the kernel's duration, best of 3 after a warm-up launch.  The values are
// meaningless (a cyclotomic squaring of a non-cyclotomic element): this times the routines in place, it does not check them.
int bn254_probe_fe_program(bn254_ctx* c, size_t n, const uint8_t* prog, size_t n_steps, float* ms) {
  if (!c || !ms || !prog || n == 0 || n > c->ws.stride || n_steps == 0 || n_steps > 4096) return BN254_E_BAD_ARGUMENT;
  for (size_t k = 0; k < n_steps; ++k) {
    const uint8_t op = prog[2 * k], arg = prog[2 * k + 1];
    if (op == 0 || op > 7) return BN254_E_BAD_ARGUMENT;
    if ((op == 1 || op == 2 || op == 4) && arg >= (BN_FE_EXACT_SLOTS > BN_FE_CHECK_SLOTS ? BN_FE_EXACT_SLOTS : BN_FE_CHECK_SLOTS)) return BN254_E_BAD_ARGUMENT;
    if (op == 6 && (arg < 1 || arg > 3)) return BN254_E_BAD_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = stage_reserve(c, 7, 2 * n_steps + 2))) return rc;
  static const uint8_t fe_end[2] = {0, 0};          // n_steps <= 4096: the program and its END pair go over in two small copies
  HIP_TRY(hipMemcpy(c->stage[7], prog, 2 * n_steps, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->stage[7] + 2 * n_steps, fe_end, 2, hipMemcpyHostToDevice));
  ScopedEvents ev;                                   // destroyed on every path out, the early error returns included
  HIP_TRY(ev.create());
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  float best = 0;
  for (int rep = 0; rep < 4 && rc == 0; ++rep) {
    HIP_TRY(hipEventRecord(e0, c->stream));
    rc = bn254_pair_fe_program(n, c->ws, c->stage[7], c->stream);
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    if (rep > 0 && (best == 0 || t < best)) best = t;
  }
  *ms = best;
  return rc;
}

// ---- test hooks --------------------------------------------------------------------------
int bn254_debug_fp_op(bn254_ctx* c, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out, uint8_t* status) {
  if (!c || (n && (!a || !out || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_a = st.in(0, a, n * 32);
  const uint8_t* d_b = b ? st.in(1, b, n * 32) : nullptr;
  uint8_t *d_out = st.out(2, n * 32, out), *d_status = st.out(3, n, status);
  if (!st.ok()) return st.rc;
  k_debug_fp_op<<<grid_for(n), BN_WAVE, 0, c->stream>>>(op, d_a, d_b, n, d_out, d_status);
  HIP_TRY(hipGetLastError());
  return st.finish();
}
int bn254_debug_fr_op(bn254_ctx* c, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
  if (!c || op < 0 || op > 6 || (n && (!a || !out)) || (n && op <= 2 && !b)) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_a = st.in(0, a, n * 32);
  const uint8_t* d_b = b ? st.in(1, b, n * 32) : nullptr;
  uint8_t* d_out = st.out(2, n * 32, out);
  if (!st.ok()) return st.rc;
  k_debug_fr_op<<<grid_for(n), BN_WAVE, 0, c->stream>>>(op, d_a, d_b, n, d_out);
  HIP_TRY(hipGetLastError());
  return st.finish();
}
int bn254_debug_lagrange_at_zero(bn254_ctx* c, const uint32_t* x, const uint64_t* seg_off, size_t n, uint8_t* out) {
  if (!c || (n && !seg_off)) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (seg_off[0] != 0 || !offsets_ok(seg_off, n) || seg_off[n] > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  const size_t m = (size_t)seg_off[n];
  if (m == 0) return 0;
  if (!x || !out) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t *d_x = st.in(0, x, m * sizeof(uint32_t)), *d_seg = st.in(1, seg_off, (n + 1) * sizeof(uint64_t));
  uint8_t* d_out = st.out(2, m * 32, out);
  if (!st.ok()) return st.rc;
  k_debug_lagrange<<<grid_for(m), BN_WAVE, 0, c->stream>>>((const uint32_t*)d_x, (const uint64_t*)d_seg, m, n, d_out);
  HIP_TRY(hipGetLastError());
  return st.finish();
}
int bn254_debug_hash_candidate(bn254_ctx* c, const uint8_t* h, size_t n, uint8_t* out, uint8_t* status) {
  if (!c || (n && (!h || !out || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_h = st.in(0, h, n * 32);
  uint8_t *d_out = st.out(2, n * 64, out), *d_status = st.out(3, n, status);
  if (!st.ok()) return st.rc;
  k_debug_hash_candidate<<<grid_for(n), BN_WAVE, 0, c->stream>>>(d_h, n, d_out, d_status);
  HIP_TRY(hipGetLastError());
  return st.finish();
}
int bn254_debug_jacobi(bn254_ctx* c, int mode, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out_value, uint8_t* out_flags) {
  if (!c || mode < 0 || mode > 2 || (n && (!a || !out_value || !out_flags)) || (n && mode == 2 && !b)) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_a = st.in(0, a, n * 32);
  const uint8_t* d_b = mode == 2 ? st.in(1, b, n * 32) : nullptr;
  uint8_t *d_value = st.out(2, n * 32, out_value), *d_flags = st.out(3, n, out_flags);
  if (!st.ok()) return st.rc;
  k_debug_jacobi<<<grid_for(n), BN_WAVE, 0, c->stream>>>(mode, d_a, d_b, n, d_value, d_flags);
  HIP_TRY(hipGetLastError());
  return st.finish();
}
// layout: 0 one lane per item, exact chain (Gt out) | 1 lane pairs, program C_FE_EXACT (Gt out) | 2 lane pairs, program C_FE_CHECK |
// 3 octet (straight-line chains below 128 items, accumulator machine from 128 on) | 4 nonet | 5 one lane per item, check chain | 6 nonet, wide form (18 lane pairs)
int bn254_debug_final_exp_limbs(bn254_ctx* c, int layout, const int32_t* limbs, size_t n, uint8_t* gt, uint8_t* status) {
  if (!c || layout < 0 || layout > 6 || (n && (!limbs || !status)) || (gt && layout > 1)) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if ((layout == 3 && !c->fits_trio) || ((layout == 4 || layout == 6) && !bn254_nonet_fits_device())) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = ws_reserve(c, n))) return rc;
  HostStaging st(c);
  const uint8_t* d_limbs = st.in(0, limbs, n * 12 * BN_LIMBS * sizeof(int32_t));
  uint8_t *d_gt = st.out(1, n * 384, gt), *d_status = st.out(2, n, status);
  if (!st.ok()) return st.rc;
  hipStream_t s = c->stream;
  k_debug_load_f<<<grid_for(n), BN_WAVE, 0, s>>>((const int32_t*)d_limbs, n, c->ws);
  switch (layout) {
    case 0: rc = launch_final_exp_lane(c, s, n, 1, 1, 1, 0, d_gt, d_status, 0, 0, nullptr, nullptr); break;
    case 1: rc = bn254_pair_final_exp_product(n, 1, c->ws, d_gt, d_status, 0, s); break;
    case 2: rc = bn254_pair_final_exp(n, c->ws, 0, d_status, nullptr, nullptr, s); break;
    case 3: rc = bn254_trio_final_exp(n, c->ws, 0, d_status, s); break;
    case 4: rc = bn254_nonet_final_exp(n, c->ws, 0, d_status, s); break;
    case 6: rc = bn254_nonet_final_exp(n, c->ws, 0, d_status, s, 1); break;
    default: rc = launch_final_exp_lane(c, s, n, 1, 1, 1, 0, nullptr, d_status, 0, 0, nullptr, nullptr); break;
  }
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return st.finish();
}
// layout: 0 one lane per item (k_debug_fq2_limbs above) | 1 one lane pair per item (bn254_pair.hip)
int bn254_debug_fq2_limbs(bn254_ctx* c, int layout, int op, const int32_t* operands, const int32_t* coef, size_t n, int32_t* out, uint8_t* flags) {
  if (!c || layout < 0 || layout > 1 || op < 0 || op >= FQ2_OP_COUNT || (n && (!operands || !coef || !out || !flags))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (n > 0xFFFFFFFFu / (BN_FQ2_HOOK_OPERANDS * BN_FQ2_HOOK_WORDS * sizeof(int32_t))) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_in = st.in(0, operands, n * BN_FQ2_HOOK_OPERANDS * BN_FQ2_HOOK_WORDS * sizeof(int32_t));
  const uint8_t* d_coef = st.in(1, coef, n * BN_FQ2_HOOK_OPERANDS * sizeof(int32_t));
  uint8_t *d_out = st.out(2, n * BN_FQ2_HOOK_WORDS * sizeof(int32_t), out), *d_flags = st.out(3, n, flags);
  if (!st.ok()) return st.rc;
  if (layout == 0) {
    k_debug_fq2_limbs<<<grid_for(n), BN_WAVE, 0, c->stream>>>(op, (const int32_t*)d_in, (const int32_t*)d_coef, n, (int32_t*)d_out, d_flags);
    HIP_TRY(hipGetLastError());
  } else {
    const int rc = bn254_pair_debug_fq2_limbs(op, (const int32_t*)d_in, (const int32_t*)d_coef, n, (int32_t*)d_out, d_flags, c->stream);
    if (rc) return rc;
  }
  return st.finish();
}
int bn254_debug_fp12_op(bn254_ctx* c, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
  if (!c || (n && (!a || !out))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_a = st.in(0, a, n * 384);
  const uint8_t* d_b = b ? st.in(1, b, n * 384) : nullptr;
  uint8_t* d_out = st.out(2, n * 384, out);
  if (!st.ok()) return st.rc;
  k_debug_fp12_op<<<grid_for(n), BN_WAVE, 0, c->stream>>>(op, d_a, d_b, n, d_out);
  HIP_TRY(hipGetLastError());
  return st.finish();
}


}  // extern "C"
