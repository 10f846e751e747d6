// The body of the developer hook bn254_debug_fq2_limbs (include/bn254_hip.h): ONE Fq2 primitive on RAW limb vectors, written against the
// fp2_* / fp_* interface only, so the same text compiles for the classic layout (bn254_devhooks.hip: one lane per item), for the pair layout
// (bn254_pair.hip: a lane pair per item, every lane holding its role's coefficient) and for the host builds of both that the bound tracker
// follows (tests/hostsim).  Every case calls the function the kernels call — no copy of any formula lives here.  Include after
// bn254_field.h, inside whatever namespace remapping the translation unit uses.
#pragma once

namespace bn254 {

// op numbers of bn254_debug_fq2_limbs (mirrored by tests/fq_limb_cases.py)
enum Fq2LimbOp {
  FQ2_ADD = 0, FQ2_SUB = 1, FQ2_NEG = 2, FQ2_DBL = 3, FQ2_CONJ = 4, FQ2_MUL_I = 5, FQ2_SELECT = 6,
  FQ2_NORM = 7, FQ2_REDUCE_WEAK = 8, FQ2_LIN2_REDUCE = 9, FQ2_LIN4_REDUCE = 10, FQ2_MUL8 = 11, FQ2_MUL_XI = 12, FQ2_MUL_XI_N = 13,
  FQ2_MUL = 14, FQ2_SQR = 15, FQ2_MUL_FP = 16, FQ2_INV = 17,
  FQ2_CANON = 18, FQ2_TO_U256 = 19, FQ2_IS_ZERO = 20, FQ2_EQ = 21, FQ2_U512_GREATER = 22, FQ2_NORM_FLOOR = 23,
  FQ2_OP_COUNT = 24
};
#define BN_FQ2_HOOK_OPERANDS 4
#define BN_FQ2_HOOK_WORDS (2 * BN_LIMBS)          // one Fq2 in the hook's buffers: re then im, 9 limbs each

// one coefficient as handed over: no decoding, no carry.  Under the bound tracker its intervals are the case's own numbers — min and max of
// limbs 0..7, |top limb|, value / q — so the tracker's precondition checks run on exactly this case.
BN_DEV Fp fq2_hook_fp(const int32_t* p) {
  Fp r;
#pragma unroll
  for (int i = 0; i < BN_LIMBS; ++i) r.v[i] = p[i];
#if defined(BN_TRACK_BOUNDS) && !defined(__HIPCC__)
  double lo = p[0], hi = p[0];
  for (int i = 1; i < BN_LIMBS - 1; ++i) { lo = std::fmin(lo, (double)p[i]); hi = std::fmax(hi, (double)p[i]); }
  long double val = 0, ql = 0;
  for (int i = BN_LIMBS - 1; i >= 0; --i) val = val * 536870912.0L + (long double)p[i];
  for (int i = 7; i >= 0; --i) ql = ql * 4294967296.0L + (long double)C_Q[i];
  // long double carries 64 bits of a 261-bit sum: an error below 2^-54 q, far inside half an ulp of a double near 80 or 600, so a case placed
  // exactly on a cap (k q with k = 80, 500, 600) comes out as exactly k, and the tracker compares with '>': it is accepted, its neighbour
  // one unit beyond the cap in the low limb likewise (it differs by 1e-77 q, which no interval arithmetic in doubles can see)
  const double v = (double)(val / ql);
  r.bd = FpBounds({lo, hi, std::fabs((double)p[BN_LIMBS - 1]), v, v});
#endif
  return r;
}
// the words of a U256 in limbs 0..7 of the hook's output (limb 8 = 0)
BN_DEV Fp fq2_hook_words(const U256& x) {
  Fp r = fp_zero();
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (int32_t)x.w[i];
  return r;
}
#if defined(BN_SPLIT_FP2)
// `role` selects the lane's coefficient on the device; the host emulation keeps both and ignores it
BN_DEV Fp2 fq2_hook_load(const int32_t* p, int role) {
  Fp2 r;
#if defined(__HIPCC__)
  r.c[0] = fq2_hook_fp(p + BN_LIMBS * role);
#else
  (void)role;
  r.c[0] = fq2_hook_fp(p); r.c[1] = fq2_hook_fp(p + BN_LIMBS);
#endif
  return r;
}
#define BN_FQ2_HOOK_COEFWISE(r, a, f) BN_FOR_ROLES(k_) (r).c[k_] = f((a).c[k_])
#else
BN_DEV Fp2 fq2_hook_load(const int32_t* p, int) { Fp2 r; r.c0 = fq2_hook_fp(p); r.c1 = fq2_hook_fp(p + BN_LIMBS); return r; }
#define BN_FQ2_HOOK_COEFWISE(r, a, f) do { (r).c0 = f((a).c0); (r).c1 = f((a).c1); } while (0)
#endif
BN_DEV Fp fq2_hook_canon(const Fp& x) { return fp_canon(x); }
BN_DEV Fp fq2_hook_to_u256(const Fp& x) { return fq2_hook_words(fp_to_u256(x)); }
BN_DEV Fp fq2_hook_norm_floor(const Fp& x) { return fp_norm_floor(x); }

// r = op(a, b, c, d; k[0..3]); s = the real coefficient of b (the scalar of FQ2_MUL_FP, the same in both lanes of a pair); flag = the answer of a
// predicate (the result is zero then).  op must be below FQ2_OP_COUNT; every lane of a launch takes the same case.
BN_DEV Fp2 fq2_hook_op(int op, const Fp2& a, const Fp2& b, const Fp2& c, const Fp2& d, const Fp& s, const int32_t* k, bool& flag) {
  Fp2 r = fp2_zero();
  flag = false;
  switch (op) {
    case FQ2_ADD: r = fp2_add(a, b); break;
    case FQ2_SUB: r = fp2_sub(a, b); break;
    case FQ2_NEG: r = fp2_neg(a); break;
    case FQ2_DBL: r = fp2_dbl(a); break;
    case FQ2_CONJ: r = fp2_conj(a); break;
    case FQ2_MUL_I: r = fp2_mul_i(a); break;
    case FQ2_SELECT: r = fp2_select(k[0] != 0, a, b); break;
    case FQ2_NORM: r = fp2_norm(a); break;
    case FQ2_REDUCE_WEAK: r = fp2_reduce_weak(a); break;
    case FQ2_LIN2_REDUCE: r = fp2_lin2_reduce(a, k[0], b, k[1]); break;
#if defined(BN_SPLIT_FP2)
    case FQ2_LIN4_REDUCE: r = fp2_lin4_reduce(a, k[0], b, k[1], c, k[2], d, k[3]); break;
#else
    case FQ2_LIN4_REDUCE:                              // the classic layout has no fp2_ wrapper: coefficient-wise
      r.c0 = fp_lin4_reduce(a.c0, k[0], b.c0, k[1], c.c0, k[2], d.c0, k[3]);
      r.c1 = fp_lin4_reduce(a.c1, k[0], b.c1, k[1], c.c1, k[2], d.c1, k[3]);
      break;
#endif
    case FQ2_MUL8: r = fp2_mul8(a); break;
    case FQ2_MUL_XI: r = fp2_mul_xi(a); break;
    case FQ2_MUL_XI_N: r = fp2_mul_xi_n(a); break;
    case FQ2_MUL: r = fp2_mul(a, b); break;
    case FQ2_SQR: r = fp2_sqr(a); break;
    case FQ2_MUL_FP: r = fp2_mul_fp(a, s); break;
    case FQ2_INV: r = fp2_inv(a); break;
    case FQ2_CANON: BN_FQ2_HOOK_COEFWISE(r, a, fq2_hook_canon); break;
    case FQ2_TO_U256: BN_FQ2_HOOK_COEFWISE(r, a, fq2_hook_to_u256); break;
    case FQ2_IS_ZERO: flag = fp2_is_zero(a); break;
    case FQ2_EQ: flag = fp2_eq(a, b); break;
    case FQ2_U512_GREATER: flag = fp2_u512_greater(a, b); break;
    default: BN_FQ2_HOOK_COEFWISE(r, a, fq2_hook_norm_floor); break;   // FQ2_NORM_FLOOR
  }
  return r;
}

}  // namespace bn254
