// Polynomials with G2 coefficients evaluated at small integer points (include/bn254_hip.h: bn254_batch_g2_poly_eval[_device],
// bn254_ctx_register_keys_commitments): out = sum_k x^k C_k by Horner's rule, acc <- x acc + C_k from the top coefficient, where
// the multiplication by a 32-bit x is a double-and-add over the Jacobian accumulator itself — about two group operations per bit of x and
// coefficient where the 256-step ladder of bn254_batch_g2_msm spends about 320.  The arithmetic and the bookkeeping of the kernels of
// bn254_polyeval.hip, shared with their host compilation for the CPU suite (tests/hostsim: plain, under -DBN_TRACK_BOUNDS and as a sanitised
// stand-alone program).
//   * DECODE, once per coefficient and not once per evaluation: Montgomery limbs (x.re | x.im | y.re | y.im, the layout of a registered key),
//     an identity byte and the decode status (flags 0: on the curve, no subgroup check).  A coefficient that does not decode is kept as the
//     generator's coordinates with the identity byte set (pe_decode); an evaluation loads a coefficient it does not own the same way
//     (pe_load), so every lane of a wave always adds a point that is on the curve.
//   * SPAN: polynomial i is [poly_off[i], poly_off[i+1]) of the m coefficients; eval_poly >= p, a reversed pair or one that runs past m reads
//     IndexOutOfBounds with no coefficients (pe_span).
//   * LANE per evaluation (pe_lane_eval): the loop bounds are the longest polynomial and the widest x of the wave; a lane whose polynomial is
//     shorter holds the identity until its own top coefficient comes by, a lane whose x is narrower doubles the identity.  x acc adds with
//     the complete jac_add (an adversarial coefficient can steer j acc into +-acc or the identity); + C_k is the mixed addition, redone with
//     the complete formula when a lane of the wave met P = +-Q (jac_accumulate).
//   * WAVE per evaluation (pe_wave_partial, pe_chunk_scalar): with L = ceil(len / 64) lane c runs Horner over the coefficients [c L, (c+1) L),
//     brings its partial sum to AFFINE form (one inversion; the windowed ladder jac_mul takes an affine base and is the ladder every other
//     call of the library walks) and multiplies it by x^(c L) mod r, computed in Fr by square-and-multiply; the 64 products meet in the
//     six-level tree of the sums (bn254_threshold.h: msm_tree_level over G2JacSlot).  A lane whose chunk is empty contributes the identity.
//   * STATUS: the lowest coefficient index with a non-zero decode status wins, as in bn254_batch_g2_msm; the output is then the identity.
// Include after bn254_hash.h, bn254_io.h, bn254_pairing.h, bn254_collect.h, bn254_fr.h, bn254_threshold.h and bn254_dealing.h.
#pragma once

namespace bn254 {

#define PE_COEFF_WORDS (4 * BN_LIMBS)

// ---- a coefficient in scratch -------------------------------------------------------------------------------------------------------------------
BN_DEV void pe_set_generator_inf(G2Affine& p) { p.x = fp2_load_const(C_G2_GEN[0]); p.y = fp2_load_const(C_G2_GEN[1]); p.inf = true; }
BN_DEV void pe_decode(int32_t* xy, uint8_t& inf, uint8_t& st, const uint8_t* point128) {
  G2Affine p;
  st = decode_g2(p, point128, 0);
  if (st != ST_OK) pe_set_generator_inf(p);
  if (p.inf) pe_set_generator_inf(p);
  const Fp c[4] = {p.x.c0, p.x.c1, p.y.c0, p.y.c1};
  for (int e = 0; e < 4; ++e)
    for (int k = 0; k < BN_LIMBS; ++k) xy[e * BN_LIMBS + k] = c[e].v[k];
  inf = p.inf;
}
// coefficient `at` when `mine`, else the generator's coordinates as the identity; st: its decode status (ST_OK when !mine)
BN_DEV void pe_load(G2Affine& p, uint8_t& st, const int32_t* xy, const uint8_t* inf, const uint8_t* coeff_st, uint64_t at, bool mine) {
  st = ST_OK;
  if (!mine) { pe_set_generator_inf(p); return; }
  const int32_t* w = xy + at * PE_COEFF_WORDS;
  p.x.c0 = fp_load_const(w); p.x.c1 = fp_load_const(w + BN_LIMBS); p.y.c0 = fp_load_const(w + 2 * BN_LIMBS); p.y.c1 = fp_load_const(w + 3 * BN_LIMBS);
  p.inf = inf[at] != 0;
  st = coeff_st[at];
}

// ---- the span of an evaluation's polynomial -----------------------------------------------------------------------------------------------------
// lo, len: the coefficients of polynomial `poly` of p over m coefficients; refused (no coefficients, IndexOutOfBounds): poly >= p, a reversed pair,
// a pair that runs past m
BN_DEV uint64_t pe_span(const uint64_t* poly_off, uint64_t p, uint64_t m, uint32_t poly, uint64_t& lo, uint8_t& st) {
  st = ST_OK;
  lo = 0;
  if (poly >= p) { st = ST_INDEX_OOB; return 0; }
  const uint64_t a = poly_off[poly], b = poly_off[(uint64_t)poly + 1];
  if (a > b || b > m) { st = ST_INDEX_OOB; return 0; }
  lo = a;
  return b - a;
}
BN_DEV int pe_bits(uint32_t x) { return x ? 32 - __builtin_clz(x) : 0; }

// ---- Horner's rule ------------------------------------------------------------------------------------------------------------------------------
// acc <- x acc, double-and-add from bit `bits - 1` (bits >= the width of x; wave-uniform).  A clear bit keeps the doubled value by select.
BN_DEV void pe_mul_small(G2Jac& acc, uint32_t x, int bits) {
  G2Jac r;
  jac_set_identity(r);
  for (int b = bits - 1; b >= 0; --b) {
    jac_dbl(r, r);
    const bool set = ((x >> b) & 1u) != 0;
    if (BN_WAVE_ANY(set)) {
      G2Jac t;
      jac_add(t, r, acc);
      jac_select(r, set, t, r);
    }
  }
  acc = r;
}
// one step: acc <- x acc + C, C the coefficient at `at` when `mine` (else the identity: the lane's value is x acc — of the identity, the
// identity).  `first`: no lane of the wave has added a coefficient yet, so there is nothing to multiply.  bad / st: the lowest index (counted
// from `lo`) with a non-zero decode status so far, and that status
BN_DEV void pe_step(G2Jac& acc, uint8_t& st, uint64_t& bad, uint32_t x, int bits, bool first, const int32_t* xy, const uint8_t* inf, const uint8_t* coeff_st,
                    uint64_t lo, uint64_t k, bool mine) {
  if (!first) pe_mul_small(acc, x, bits);
  G2Affine c;
  uint8_t cst;
  pe_load(c, cst, xy, inf, coeff_st, lo + k, mine);
  if (cst != ST_OK && k < bad) { bad = k; st = cst; }
  jac_accumulate(acc, c);
}
// lane per evaluation: the whole polynomial [lo, lo + len).  max_len, bits: the wave's (on the host: the lane's own)
BN_DEV void pe_lane_eval(G2Jac& acc, uint8_t& st, uint32_t x, const int32_t* xy, const uint8_t* inf, const uint8_t* coeff_st, uint64_t lo, uint64_t len,
                         uint64_t max_len, int bits) {
  uint64_t bad = UINT64_MAX;
  st = ST_OK;
  jac_set_identity(acc);
  for (uint64_t k = max_len; k-- > 0;) pe_step(acc, st, bad, x, bits, k + 1 == max_len, xy, inf, coeff_st, lo, k, k < len);
}
// wave per evaluation, lane `lane` of BN_CL_WAVE: Horner over its chunk of L = ceil(len / 64) coefficients — the value of the chunk's own
// polynomial at x, still to be multiplied by x^(lane L)
BN_DEV uint64_t pe_chunk_len(uint64_t len) { return (len + BN_CL_WAVE - 1) / BN_CL_WAVE; }
BN_DEV void pe_wave_partial(G2Jac& acc, uint8_t& st, uint64_t& bad, uint32_t x, const int32_t* xy, const uint8_t* inf, const uint8_t* coeff_st, uint64_t lo,
                            uint64_t len, unsigned lane) {
  const uint64_t L = pe_chunk_len(len), base = (uint64_t)lane * L;
  const int bits = pe_bits(x);
  bad = UINT64_MAX;
  st = ST_OK;
  jac_set_identity(acc);
  for (uint64_t j = L; j-- > 0;) pe_step(acc, st, bad, x, bits, j + 1 == L, xy, inf, coeff_st, lo, base + j, base + j < len);
}
// x^e mod r as plain words, e < 2^64: square-and-multiply in Fr from the top bit of the wave's widest exponent (e_bits)
BN_DEV void pe_chunk_scalar(uint32_t* k, uint32_t x, uint64_t e, int e_bits) {
  const Fr bx = fr_from_u32(x);
  Fr acc = fr_one();
  for (int b = e_bits - 1; b >= 0; --b) {
    acc = fr_mul(acc, acc);
    if ((e >> b) & 1u) acc = fr_mul(acc, bx);
  }
  fr_to_words(k, acc);
}
BN_DEV int pe_bits64(uint64_t e) { return e ? 64 - __builtin_clzll(e) : 0; }
// the lane's contribution: x^(lane L) times its partial, through the affine form and the 256-step ladder.  The identity walks the ladder under
// the generator's coordinates (bn254_dealing.h: g2msm_ladder)
BN_DEV void pe_wave_scale(G2Jac& out, const G2Jac& partial, uint32_t x, uint64_t len, unsigned lane) {
  const uint64_t L = pe_chunk_len(len);
  uint32_t k[8];
  pe_chunk_scalar(k, x, (uint64_t)lane * L, pe_bits64((uint64_t)(BN_CL_WAVE - 1) * L));
  G2Affine a;
  jac_to_affine(a, partial);
  if (a.inf) pe_set_generator_inf(a);
  jac_mul(out, a, k);
}

}  // namespace bn254
