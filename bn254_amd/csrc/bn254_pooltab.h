// The subset-sum tables of the aggregate verify's pools (include/bn254_hip.h: bn254_batch_aggregate_verify, bn254_ctx_register_pools): the
// arithmetic of their builders, one lane at a time, shared by the device kernels (bn254_group.hip: k_pool_subsets_g2 / _g1, k_pool_pairs_g1,
// k_pool_quads_g1, k_pool_widen_g1 / _g2 are thin wrappers around the *_lane functions below) and their host compilation for the CPU suite
// (tests/hostsim, plain and under -DBN_TRACK_BOUNDS).
//   * TABLES.  In every table bit b of `mask` selects signer W * window + b; a signer that is missing (>= n_signers), refused (decode status
//     != 0) or the identity counts as the identity.
//       T8 keys        entry g * 256 + mask                       8 signers per window    pt_subsets_g2_lane   (from the key pool)
//       T2 signatures  entry (m * groups2 + pair) * 4 + mask      2                       pt_pairs_g1_lane     (from the signature pool)
//       T4 signatures  entry (m * groups4 + g) * 16 + mask        4                       pt_quads_g1_lane     (T2 + T2); pt_subsets_g1_lane (from the pool)
//       T8 signatures  entry (m * n_groups + g) * 256 + mask      8                       pt_widen_g1_lane     (T4 + T4)
//       T16 keys       entry k * 65536 + mask                     16                      pt_widen_g2_lane     (T8 + T8)
//   * WIDENING (pool_widen_lane): dst[hi * 2^w + lo] = src[group 2k][lo] + src[group 2k + 1][hi] — ONE affine addition per entry.  A lane owns
//     one `hi` (its operand A) and walks its `lo` values in batches whose denominators x_B - x_A share ONE inversion (Montgomery's trick: prefix
//     products up, the inverse peeled off on the way down; the B points are read twice, an L2 hit, instead of being kept in registers).  An
//     entry with an identity operand is a copy; the rare lo with x_B = x_A (B = +-A: a pool that holds a point twice, or a point and its
//     negative, or a sum that equals another) takes the complete Jacobian formula and an inversion of its own.
//   * STORED WORDS.  A coordinate in a table (and in the decoded pools the first stage reads) is as the kernels left it: carried limbs
//     (|limb| <= 2^28) of a value v with |v| <= PT_WORD_VMAX * q — NOT canonical: a chord's coordinates are weakly reduced (|v| < 0.7 q), a
//     Jacobian sum's come out of a product, a decoded point's are in [0, q).  pt_store_fp checks this under the bound tracker of the host
//     compilation and pt_load_fp assumes it, so that one tracked pass of each flow is a proof for every chain T2 -> T4 -> T8, T8 -> T16 and
//     for the consumers' additions (bn254_pair.hip: k_aggregate_pair reads the same records).
// Written against a TABLE ACCESSOR — any struct with `int32_t* planes; uint8_t* st; uint32_t g2;` in the record layout of bn254_ws.h's Pool,
// which is what the kernels pass; PtTab is the host's.  Include after bn254_pairing.h.  The builders run in the one-lane layout of Fq2; in
// the pair layout (BN_SPLIT_FP2) only the accessors and the record source PtRec are available: the consumer's side.
#pragma once

namespace bn254 {

#define PT_HALF_WORDS 20                   /* = BN_POOL_HALF_WORDS: x (9 words) | y (9) | 2 pad */
struct PtTab { int32_t* planes; uint8_t* st; uint32_t g2; };

// word offset of coordinate e of entry j.  G1: 0 = x, 1 = y; G2: 0 = x.re, 1 = x.im, 2 = y.re, 3 = y.im, the real parts in the first half
template <class Tab> BN_DEV size_t pt_word(const Tab& p, int e, size_t j) {
  return p.g2 ? j * (2 * PT_HALF_WORDS) + (size_t)((e & 1) * PT_HALF_WORDS + (e >> 1) * BN_LIMBS) : j * PT_HALF_WORDS + (size_t)(e * BN_LIMBS);
}
// the stored-word contract: |value| <= PT_WORD_VMAX q on carried limbs, checked at every store, assumed at every load
#define PT_WORD_VMAX 1.0
BN_DEV Fp pt_load_words(const int32_t* w) {
  Fp r;
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) r.v[k] = w[k];
  BN_TRK(bn_set_tight(r, -PT_WORD_VMAX, PT_WORD_VMAX));
  return r;
}
template <class Tab> BN_DEV Fp pt_load_fp(const Tab& p, int e, size_t j) { return pt_load_words(p.planes + pt_word(p, e, j)); }
template <class Tab> BN_DEV void pt_store_fp(const Tab& p, int e, size_t j, const Fp& a) {
  BN_TRK(if (a.bd.lo < -BN_T || a.bd.hi > BN_T || a.bd.vlo < -PT_WORD_VMAX || a.bd.vhi > PT_WORD_VMAX) bn_bound_fail("pool table entry outside the stored-word contract", bn_vabs(a)));
  int32_t* w = p.planes + pt_word(p, e, j);
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) w[k] = a.v[k];
}

#if defined(BN_SPLIT_FP2)
// a table record as the source of an in-place addition in the pair layout (bn254_curve.h: jac_accumulate_from), read as k_aggregate_pair's
// PoolRec reads it — a G1 record, or the lane's half of a G2 record: x at word 0, y at word 9 — under the stored-word contract
#if defined(__HIPCC__)
#define PT_MEMBER __device__ __forceinline__
#else
#define PT_MEMBER inline
#endif
struct PtRec {
  const int32_t* p;
  bool inf;
  PT_MEMBER void operator()(G1Affine& q) const { q.x = pt_load_words(p); q.y = pt_load_words(p + BN_LIMBS); q.inf = inf; }
  PT_MEMBER void operator()(G2Affine& q) const {          // p = the record: a lane reads the half of its role
    BN_FOR_ROLES(k) { const int32_t* h = p + bn_role_index(k) * PT_HALF_WORDS; q.x.c[k] = pt_load_words(h); q.y.c[k] = pt_load_words(h + BN_LIMBS); }
    q.inf = inf;
  }
};
#else

template <class Tab> BN_DEV void pool_load_aff(const Tab& p, size_t j, G1Affine& q) { q.x = pt_load_fp(p, 0, j); q.y = pt_load_fp(p, 1, j); q.inf = (p.st[j] & 0x80) != 0; }
template <class Tab> BN_DEV void pool_load_aff(const Tab& p, size_t j, G2Affine& q) {
  q.x.c0 = pt_load_fp(p, 0, j); q.x.c1 = pt_load_fp(p, 1, j); q.y.c0 = pt_load_fp(p, 2, j); q.y.c1 = pt_load_fp(p, 3, j);
  q.inf = (p.st[j] & 0x80) != 0;
}
template <class Tab> BN_DEV void pool_store_aff(const Tab& p, size_t j, const G1Affine& q) { pt_store_fp(p, 0, j, q.x); pt_store_fp(p, 1, j, q.y); p.st[j] = q.inf ? 0x80 : 0; }
template <class Tab> BN_DEV void pool_store_aff(const Tab& p, size_t j, const G2Affine& q) {
  pt_store_fp(p, 0, j, q.x.c0); pt_store_fp(p, 1, j, q.x.c1); pt_store_fp(p, 2, j, q.y.c0); pt_store_fp(p, 3, j, q.y.c1);
  p.st[j] = q.inf ? 0x80 : 0;
}
template <class F> BN_DEV void aff_select(Affine<F>& r, bool c, const Affine<F>& a, const Affine<F>& b) {
  r.x = f_select(c, a.x, b.x); r.y = f_select(c, a.y, b.y); r.inf = c ? a.inf : b.inf;
}
// one lane: dst[dst0 + lo] = src[b0 + lo] + A for NLO consecutive lo (an entry of src may be the identity: the empty subset, or a sum that
// cancelled).  A.inf set: A's coordinates are a stand-in (the generator's), never (0, 0).
template <class F, int NLO, int BATCH = 8, class Tab> BN_DEV void pool_widen_lane(bool live, const Tab& src, size_t b0, Affine<F> A, const Tab& dst, size_t dst0) {
  static_assert(NLO % BATCH == 0, "whole batches");
  for (int base = 0; base < NLO; base += BATCH) {
    F d[BATCH], pre[BATCH];
    bool exc[BATCH];
#pragma unroll
    for (int i = 0; i < BATCH; ++i) {
      Affine<F> B;
      pool_load_aff(src, b0 + base + i, B);
      d[i] = f_norm(f_sub(B.x, A.x));
      const bool zero = f_is_zero(d[i]);
      exc[i] = zero && !A.inf && !B.inf;              // B = +-A
      if (zero || A.inf || B.inf) f_set_one(d[i]);    // keeps the batch's product invertible; the chord of such an entry is not used
      pre[i] = i ? f_mul(pre[i - 1], d[i]) : d[i];
    }
    F inv = f_inv(pre[BATCH - 1]);
#pragma unroll
    for (int i = BATCH - 1; i >= 0; --i) {
      const F dinv = i ? f_mul(inv, pre[i - 1]) : inv;
      if (i) inv = f_mul(inv, d[i]);
      Affine<F> B, R;
      pool_load_aff(src, b0 + base + i, B);
      aff_add_given_inv(R, A, B, dinv);
      aff_select(R, B.inf, A, R);                     // identity operands: copies
      aff_select(R, A.inf, B, R);
      if (BN_WAVE_ANY(exc[i])) {                      // rare: the complete formula (and an inversion of its own) for the lanes that met B = +-A
        Jac<F> J;
        Affine<F> Bc = B, C;
        jac_from_affine(J, A);
        Bc.inf = !exc[i];                             // the other lanes add nothing here
        jac_madd(J, J, Bc);
        jac_to_affine(C, J);
        if (exc[i]) R = C;
      }
      if (live) pool_store_aff(dst, dst0 + base + i, R);
    }
  }
}

// ---- the builders, one lane each: `lane` = the global thread index of the kernel; a lane past the end computes with entry 0 and stores nothing
// T8 keys: the sums of all 255 non-empty subsets of every group of 8 consecutive keys (~4 additions + one inversion per entry).  lane = entry
template <class Tab> BN_DEV void pt_subsets_g2_lane(size_t j, const Tab& pk_pool, size_t n_signers, size_t n_groups, const Tab& sub) {
  const bool live = j < n_groups * 256;
  const size_t g = (live ? j : 0) >> 8;
  const unsigned mask = (unsigned)(j & 255u);
  G2Jac acc;
  jac_set_identity(acc);
  for (int b = 0; b < 8; ++b) {                      // wave-uniform: jac_accumulate votes across the wave
    const size_t sgn = g * 8 + b;
    const size_t ss = sgn < n_signers ? sgn : 0;
    const uint8_t st = pk_pool.st[ss];
    G2Affine p;
    p.x.c0 = pt_load_fp(pk_pool, 0, ss); p.x.c1 = pt_load_fp(pk_pool, 1, ss);
    p.y.c0 = pt_load_fp(pk_pool, 2, ss); p.y.c1 = pt_load_fp(pk_pool, 3, ss);
    p.inf = !live || !((mask >> b) & 1u) || sgn >= n_signers || st != 0;       // st: 0x80 = identity entry, low bits = decode error
    jac_accumulate(acc, p);
  }
  G2Affine a;
  jac_to_affine(a, acc);
  if (!live) return;
  pt_store_fp(sub, 0, j, a.x.c0); pt_store_fp(sub, 1, j, a.x.c1);
  pt_store_fp(sub, 2, j, a.y.c0); pt_store_fp(sub, 3, j, a.y.c1);
  sub.st[j] = a.inf ? 0x80 : 0;
}
// T4 signatures straight from the pool: four accumulations and an inversion per ENTRY (the route when the pair table cannot be allocated)
template <class Tab> BN_DEV void pt_subsets_g1_lane(size_t j, const Tab& sig_pool, size_t n_signers, size_t groups4, size_t n_msgs, const Tab& sub) {
  const bool live = j < n_msgs * groups4 * 16;
  const size_t jj = live ? j : 0;
  const unsigned mask = (unsigned)(jj & 15u);
  const size_t g = (jj >> 4) % groups4, m = (jj >> 4) / groups4;
  G1Jac acc;
  jac_set_identity(acc);
  for (int b = 0; b < 4; ++b) {                      // wave-uniform
    const size_t sgn = g * 4 + b;
    const size_t sj = m * n_signers + (sgn < n_signers ? sgn : 0);
    const uint8_t st = sig_pool.st[sj];
    G1Affine p;
    p.x = pt_load_fp(sig_pool, 0, sj); p.y = pt_load_fp(sig_pool, 1, sj);
    p.inf = !live || !((mask >> b) & 1u) || sgn >= n_signers || st != 0;
    jac_accumulate(acc, p);
  }
  G1Affine a;
  jac_to_affine(a, acc);
  if (!live) return;
  pt_store_fp(sub, 0, j, a.x); pt_store_fp(sub, 1, j, a.y);
  sub.st[j] = a.inf ? 0x80 : 0;
}
// T16 keys: T16[k][hi * 256 + lo] = T8[2k][lo] + T8[2k + 1][hi]; lane = (k, hi, block of 32 lo values).  A chunk whose second group does not
// exist (an odd number of groups) has nothing to add: every hi copies T8[2k][lo]
#define BN_WIDEN_G2_NLO 32
template <class Tab> BN_DEV void pt_widen_g2_lane(size_t lane, const Tab& t8, size_t n_groups, size_t n_chunks, const Tab& t16) {
  constexpr size_t BLK = 256 / BN_WIDEN_G2_NLO;
  const bool live = lane < n_chunks * 256 * BLK;
  const size_t ll = live ? lane : 0, blk = ll % BLK, hi = (ll / BLK) & 255u, k = ll / (BLK * 256);
  const bool has_hi = 2 * k + 1 < n_groups;
  G2Affine A;
  pool_load_aff(t8, (has_hi ? 2 * k + 1 : 2 * k) * 256 + hi, A);
  A.inf = A.inf || !has_hi || hi == 0;
  if (A.inf) { A.x = fp2_load_const(C_G2_GEN[0]); A.y = fp2_load_const(C_G2_GEN[1]); }
  pool_widen_lane<Fp2, BN_WIDEN_G2_NLO>(live, t8, 2 * k * 256 + blk * BN_WIDEN_G2_NLO, A, t16, k * 65536 + hi * 256 + blk * BN_WIDEN_G2_NLO);
}
// T8 signatures, per message: T8[m][g][hi * 16 + lo] = T4[m][2g][lo] + T4[m][2g + 1][hi]; lane = (m, g, hi)
template <class Tab> BN_DEV void pt_widen_g1_lane(size_t lane, const Tab& t4, size_t groups4, size_t n_groups, size_t n_msgs, const Tab& t8) {
  const bool live = lane < n_msgs * n_groups * 16;
  const size_t ll = live ? lane : 0, hi = ll & 15u, g = (ll >> 4) % n_groups, m = (ll >> 4) / n_groups;
  G1Affine A;
  pool_load_aff(t4, (m * groups4 + 2 * g + 1) * 16 + hi, A);
  A.inf = A.inf || hi == 0;
  if (A.inf) { A.x = fp_load_const(C_G1_GEN[0]); A.y = fp_load_const(C_G1_GEN[1]); }
  pool_widen_lane<Fp, 16>(live, t4, (m * groups4 + 2 * g) * 16, A, t8, (m * n_groups + g) * 256 + hi * 16);
}
// T2 signatures: T2[m][pair][mask] = {O, s0, s1, s0 + s1} for every pair of consecutive signers (one complete addition and one inversion per
// PAIR); lane = (m, pair)
template <class Tab> BN_DEV void pt_pairs_g1_lane(size_t lane, const Tab& sig_pool, size_t n_signers, size_t groups2, size_t n_msgs, const Tab& t2) {
  const bool live = lane < n_msgs * groups2;
  const size_t ll = live ? lane : 0, g = ll % groups2, m = ll / groups2;
  G1Affine s[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const size_t sgn = 2 * g + b, sj = m * n_signers + (sgn < n_signers ? sgn : 0);
    s[b].x = pt_load_fp(sig_pool, 0, sj); s[b].y = pt_load_fp(sig_pool, 1, sj);
    s[b].inf = sgn >= n_signers || sig_pool.st[sj] != 0;          // st: 0x80 = identity entry, low bits = decode error (counts as the identity here)
    if (s[b].inf) { s[b].x = fp_load_const(C_G1_GEN[0]); s[b].y = fp_load_const(C_G1_GEN[1]); }
  }
  G1Jac J;
  G1Affine sum, none;
  jac_from_affine(J, s[0]);
  jac_madd(J, J, s[1]);
  jac_to_affine(sum, J);
  none.x = fp_zero(); none.y = fp_zero(); none.inf = true;
  if (!live) return;
  pool_store_aff(t2, 4 * lane + 0, none);
  pool_store_aff(t2, 4 * lane + 1, s[0]);
  pool_store_aff(t2, 4 * lane + 2, s[1]);
  pool_store_aff(t2, 4 * lane + 3, sum);
}
// T4 signatures: T4[hi * 4 + lo] = T2[pair 2g][lo] + T2[pair 2g + 1][hi], batches of 4; lane = (m, g, hi)
template <class Tab> BN_DEV void pt_quads_g1_lane(size_t lane, const Tab& t2, size_t groups2, size_t groups4, size_t n_msgs, const Tab& t4) {
  const bool live = lane < n_msgs * groups4 * 4;
  const size_t ll = live ? lane : 0, hi = ll & 3u, g = (ll >> 2) % groups4, m = (ll >> 2) / groups4;
  G1Affine A;
  pool_load_aff(t2, (m * groups2 + 2 * g + 1) * 4 + hi, A);
  if (A.inf) { A.x = fp_load_const(C_G1_GEN[0]); A.y = fp_load_const(C_G1_GEN[1]); }
  pool_widen_lane<Fp, 4, 4>(live, t2, (m * groups2 + 2 * g) * 4, A, t4, (m * groups4 + g) * 16 + hi * 4);
}
#endif  // BN_SPLIT_FP2

}  // namespace bn254
