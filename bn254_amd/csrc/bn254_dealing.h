// The segmented scalar-weighted sum in G2 and the check of a t-of-n dealing over the registered keys (include/bn254_hip.h:
// bn254_batch_g2_msm[_device], bn254_ctx_check_dealing, bn254_debug_dealing_coefficients): the arithmetic and the bookkeeping of the kernels of
// bn254_dealing.hip, shared with their host compilation for the CPU suite (tests/hostsim: plain, under -DBN_TRACK_BOUNDS
// and as a sanitised stand-alone program).
//   * TERM: k_s P_s by the 256-step ladder of bn254_batch_g2_mul (jac_mul) into a Jacobian scratch entry per term, no inversion (g2msm_term).
//     The point is decoded from 128 bytes with flags 0, or read from the registered table (g2msm_term_key: key_xy / key_inf as registration
//     left them).  A masked or non-decoding term walks the generator's coordinates with the identity flag set, so the wave stays convergent.
//   * SUM: the G1 sum's bodies over G2Jac (bn254_threshold.h: msm_seg_len, msm_lane_sum, msm_wave_partial, msm_tree_level): a lane walks a
//     short segment in order, a wave folds a long one through the six-level tree; one inversion per segment (g2msm_encode).
//   * COEFFICIENTS of the degree check.  Key j stands for x_j = j + 1, so x_j - x_i = j - i and every product of differences is a factorial:
//       prod_{i<t, i != k} (x_k - x_i) = (-1)^(t-1-k) k! (t-1-k)!            prod_{i<t} (x_j - x_i) = j! / (j-t)!   (j >= t)
//       L_k(x_j) = j! / ((j-t)! (j-k)) / ((-1)^(t-1-k) k! (t-1-k)!)           lambda_k = (-1)^k t! / ((k+1) k! (t-1-k)!)
//     With fact[m] = m! (dl_fact_*: a chunked product scan, 64 lanes), inv[m] = 1/m and w_j = rho_j j!/(j-t)! (dl_tables: one inversion per
//     entry, a lane each), key k < t costs n - t products for sum_j w_j inv[j-k] and one inversion (dl_coeff): O(t (n-t)) products and O(n)
//     inversions in all.  Everything is in Montgomery form; the coefficients leave as 32 big-endian bytes, reduced.
//   * SETTLE: the lowest key with a non-zero registration status, threshold > n, the second sum not the identity, or the group key (dl_settle).
// Include after bn254_hash.h (rand_scalar), bn254_collect.h, bn254_fr.h and bn254_threshold.h.
#pragma once

namespace bn254 {

// ---- the weighted sum in G2: term and encode (the sums are bn254_threshold.h's, over G2Jac) --------------------------------------------------------
BN_DEV void g2msm_ladder(G2Jac& out, G2Affine& p, bool usable, const uint8_t* scalar32, bool reduce) {
  if (!usable) { p.x = fp2_load_const(C_G2_GEN[0]); p.y = fp2_load_const(C_G2_GEN[1]); p.inf = true; }
  uint32_t k[8];
  for (int i = 0; i < 8; ++i) k[i] = 0;
  if (usable) scalar_from_be(k, scalar32, reduce);
  jac_mul(out, p, k);
}
// term s = k P from 128 bytes, decoded with flags 0 as k_g2_mul and k_g2_sum decode them.  !take, or a point that does not decode: the identity
BN_DEV void g2msm_term(G2Jac& out, uint8_t& st, const uint8_t* point128, const uint8_t* scalar32, bool reduce, bool take) {
  G2Affine p;
  st = ST_OK;
  if (take) st = decode_g2(p, point128, 0);
  g2msm_ladder(out, p, take && st == ST_OK, scalar32, reduce);
}
// ... from the registered table: the 4 x BN_LIMBS words of one key (x.re | x.im | y.re | y.im) and its identity byte.  Registration decoded the
// key; a key with a non-zero status never gets here (dl_settle reports it before anything is summed).
BN_DEV void g2msm_term_key(G2Jac& out, const int32_t* xy, bool inf, const uint8_t* scalar32, bool take) {
  G2Affine p;
  p.x.c0 = fp_load_const(xy); p.x.c1 = fp_load_const(xy + BN_LIMBS); p.y.c0 = fp_load_const(xy + 2 * BN_LIMBS); p.y.c1 = fp_load_const(xy + 3 * BN_LIMBS);
  p.inf = inf;
  g2msm_ladder(out, p, take, scalar32, false);
}
// the sum as the caller gets it: the identity (128 zero bytes) under a non-zero status
BN_DEV void g2msm_encode(uint8_t* out128, const G2Jac& acc, uint8_t st) {
  G2Affine r;
  jac_to_affine(r, acc);
  if (st != ST_OK) r.inf = true;
  encode_g2(out128, r);
}
// the slot of a partial sum in LDS: a G2Jac (6 x 9 limbs = 216 B) and a pad word, so the stride in words is odd (55) as ClJacSlot's is
struct G2JacSlot { G2Jac v; int32_t pad; };

// ---- the coefficients of the degree check ------------------------------------------------------------------------------------------------------
// fact[0 .. n1): lane `lane` of BN_CL_WAVE owns the entries [lane per, lane per + per), per = ceil(n1 / 64).  Three steps: every lane the
// product of its entries (0 counts as 1); ONE lane the exclusive prefix products of the 64 partials, in place; every lane its entries.
BN_DEV void dl_fact_range(uint32_t n1, unsigned lane, uint32_t& lo, uint32_t& hi) {
  const uint32_t per = (n1 + BN_CL_WAVE - 1) / BN_CL_WAVE;
  const uint64_t a = (uint64_t)lane * per, b = a + per;
  lo = a < n1 ? (uint32_t)a : n1;
  hi = b < n1 ? (uint32_t)b : n1;
}
BN_DEV Fr dl_fact_partial(uint32_t n1, unsigned lane) {
  uint32_t lo, hi;
  dl_fact_range(n1, lane, lo, hi);
  Fr p = fr_one();
  for (uint32_t m = lo; m < hi; ++m)
    if (m) p = fr_mul(p, fr_from_u32(m));
  return p;
}
BN_DEV void dl_fact_prefix(Fr* part) {
  Fr run = fr_one();
  for (unsigned l = 0; l < BN_CL_WAVE; ++l) { const Fr own = part[l]; part[l] = run; run = fr_mul(run, own); }
}
BN_DEV void dl_fact_write(Fr* fact, uint32_t n1, unsigned lane, const Fr& prefix) {
  uint32_t lo, hi;
  dl_fact_range(n1, lane, lo, hi);
  Fr run = prefix;
  for (uint32_t m = lo; m < hi; ++m) {
    if (m) run = fr_mul(run, fr_from_u32(m));
    fact[m] = run;
  }
}
// rho_j: the 128-bit weight of index j under the seed, the derivation of bn254_batch_verify_randomized (bn254_hash.h: rand_scalar)
BN_DEV Fr dl_rho(const uint32_t* seed_be, uint64_t j) {
  uint32_t k[4];
  rand_scalar(k, seed_be, j, false);
  Fr a = fr_zero();
  for (int i = 0; i < 4; ++i) a.w[i] = k[i];
  return fr_to_mont(a);
}
// entry m of the tables, m in [0, n]: inv[m] = 1/m (0 for m = 0); for t <= m < n also w[m - t] = rho_m m!/(m-t)! and c_m = rho_m as bytes
BN_DEV void dl_tables(Fr* inv, Fr* w, uint8_t* coeff_be, const Fr* fact, const uint32_t* seed_be, uint32_t n, uint32_t t, uint32_t m) {
  inv[m] = m ? fr_inv(fr_from_u32(m)) : fr_zero();
  if (m < t || m >= n) return;
  const Fr rho = dl_rho(seed_be, m);
  w[m - t] = fr_mul(rho, fr_mul(fact[m], fr_inv(fact[m - t])));
  fr_to_be(coeff_be + 32 * (size_t)m, rho);
}
// key k < t: lambda_k of the points 1 .. t, and c_k = -sum_{j=t}^{n-1} rho_j L_k(x_j)
BN_DEV void dl_coeff(Fr& lambda, Fr& ck, const Fr* fact, const Fr* inv, const Fr* w, uint32_t n, uint32_t t, uint32_t k) {
  Fr s = fr_zero();
  for (uint32_t j = t; j < n; ++j) s = fr_add(s, fr_mul(w[j - t], inv[j - k]));
  const Fr e = fr_inv(fr_mul(fact[k], fact[t - 1 - k]));
  lambda = fr_mul(fr_mul(fact[t], inv[k + 1]), e);
  if (k & 1u) lambda = fr_neg(lambda);
  ck = fr_mul(s, e);
  if (((t - 1 - k) & 1u) == 0) ck = fr_neg(ck);
}

// ---- the verdict -------------------------------------------------------------------------------------------------------------------------------
// the lowest key with a non-zero registration status among those lane `lane` of BN_CL_WAVE looks at (UINT32_MAX: none), and the fold of two such
BN_DEV void dl_scan_lane(uint32_t& key, uint8_t& st, const uint8_t* key_st, uint32_t n, unsigned lane) {
  key = UINT32_MAX;
  st = ST_OK;
  for (uint64_t j = lane; j < n; j += BN_CL_WAVE)
    if (key_st[j] != ST_OK) { key = (uint32_t)j; st = key_st[j]; break; }
}
BN_DEV void dl_scan_fold(uint32_t& key, uint8_t& st, uint32_t other_key, uint8_t other_st) {
  if (other_key < key) { key = other_key; st = other_st; }
}
// what the host reads: 128 + 4 + 1 bytes
struct DlResult { uint8_t pk[128]; uint32_t bad_key; uint8_t status; };
// the four outcomes, in order.  sums: the two segments' encodings (K, then the check's sum), sum_st their statuses — read only when the sums ran
BN_DEV void dl_settle(DlResult& r, uint32_t bad_key, uint8_t bad_st, bool t_over, const uint8_t* sums256, const uint8_t* sum_st) {
  uint32_t* pk = (uint32_t*)r.pk;
  for (int k = 0; k < 32; ++k) pk[k] = 0;
  r.bad_key = bad_key;
  if (bad_key != UINT32_MAX) { r.status = bad_st; return; }
  r.status = ST_VERIFICATION_FAILED;
  if (t_over) return;
  const uint32_t* s = (const uint32_t*)sums256;
  uint32_t any = (uint32_t)sum_st[0] | sum_st[1];
  for (int k = 32; k < 64; ++k) any |= s[k];
  if (any) return;
  r.status = ST_OK;
  for (int k = 0; k < 32; ++k) pk[k] = s[k];
}

}  // namespace bn254
