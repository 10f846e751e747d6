// Fr: arithmetic mod the group order r = C_ORDER_R, for the Lagrange coefficients of threshold signatures (bn254_threshold.h; include/bn254_hip.h:
// bn254_batch_threshold_combine_keyed).  Plain C++: 8 x 32-bit words, little-endian, 64-bit accumulation, Montgomery form with R = 2^256
// (constants: gen_constants.py -> BN_FR_N0, C_FR_R2, C_FR_ONE).  Not a hot loop — a coefficient is about 2t + 400 products beside a ladder of
// 128 doublings and 66 additions in Fq — so there is no assembly here, and the header compiles for the host as it stands (tests/hostsim).
// Every function takes and returns REDUCED values (< r) unless it says otherwise; r < 2^254, so a sum of two fits 256 bits.
// Include after bn254_io.h (u256_from_be, scalar_from_be).
#pragma once

namespace bn254 {

struct Fr { uint32_t w[8]; };

BN_DEV Fr fr_zero() {
  Fr r;
  for (int i = 0; i < 8; ++i) r.w[i] = 0;
  return r;
}
BN_DEV Fr fr_one() {                                          // Montgomery form
  Fr r;
  for (int i = 0; i < 8; ++i) r.w[i] = C_FR_ONE[i];
  return r;
}
BN_DEV bool fr_is_zero(const Fr& a) {
  uint32_t any = 0;
  for (int i = 0; i < 8; ++i) any |= a.w[i];
  return any == 0;
}
// a - r when a >= r (a < 2r)
BN_DEV void fr_cond_sub(Fr& a) {
  if (!u256_geq(a.w, C_ORDER_R)) return;
  uint32_t bw = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)a.w[i] - C_ORDER_R[i] - bw;
    a.w[i] = (uint32_t)d; bw = (uint32_t)(d >> 63);
  }
}
BN_DEV Fr fr_add(const Fr& a, const Fr& b) {
  Fr r;
  uint64_t cy = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)a.w[i] + b.w[i] + cy;
    r.w[i] = (uint32_t)t; cy = t >> 32;
  }
  fr_cond_sub(r);
  return r;
}
BN_DEV Fr fr_sub(const Fr& a, const Fr& b) {
  Fr r;
  uint32_t bw = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)a.w[i] - b.w[i] - bw;
    r.w[i] = (uint32_t)d; bw = (uint32_t)(d >> 63);
  }
  if (bw) {                                                   // negative: + r
    uint64_t cy = 0;
    for (int i = 0; i < 8; ++i) {
      const uint64_t t = (uint64_t)r.w[i] + C_ORDER_R[i] + cy;
      r.w[i] = (uint32_t)t; cy = t >> 32;
    }
  }
  return r;
}
BN_DEV Fr fr_neg(const Fr& a) { return fr_sub(fr_zero(), a); }
// Montgomery product a b / 2^256 mod r, word by word (CIOS).  One operand may be any 256-bit value as long as the other is reduced: the
// running sum stays below 2r, so one conditional subtraction ends it.
BN_DEV Fr fr_mul(const Fr& a, const Fr& b) {
  uint32_t t[10];
  for (int i = 0; i < 10; ++i) t[i] = 0;
  for (int i = 0; i < 8; ++i) {
    uint64_t c = 0;
    for (int j = 0; j < 8; ++j) {
      const uint64_t s = (uint64_t)t[j] + (uint64_t)a.w[j] * b.w[i] + c;      // <= 2^64 - 1
      t[j] = (uint32_t)s; c = s >> 32;
    }
    uint64_t s = (uint64_t)t[8] + c;
    t[8] = (uint32_t)s; t[9] = (uint32_t)(s >> 32);
    const uint32_t m = t[0] * BN_FR_N0;
    s = (uint64_t)t[0] + (uint64_t)m * C_ORDER_R[0];
    c = s >> 32;
    for (int j = 1; j < 8; ++j) {
      s = (uint64_t)t[j] + (uint64_t)m * C_ORDER_R[j] + c;
      t[j - 1] = (uint32_t)s; c = s >> 32;
    }
    s = (uint64_t)t[8] + c;
    t[7] = (uint32_t)s; t[8] = t[9] + (uint32_t)(s >> 32);
  }
  Fr r;
  for (int i = 0; i < 8; ++i) r.w[i] = t[i];                  // < 2r < 2^255: t[8] == 0
  fr_cond_sub(r);
  return r;
}
// plain value (any 256 bits) -> Montgomery form, reduced; and back
BN_DEV Fr fr_to_mont(const Fr& a) {
  Fr r2;
  for (int i = 0; i < 8; ++i) r2.w[i] = C_FR_R2[i];
  return fr_mul(a, r2);
}
BN_DEV Fr fr_from_mont(const Fr& a) {
  Fr one = fr_zero();
  one.w[0] = 1;
  return fr_mul(a, one);
}
// loads, into Montgomery form: a 32-bit value (< r as it stands), and 32 big-endian bytes reduced like scalar_from_be(.., true).  (The
// Lagrange coefficients do not load their points: they feed them to fr_mul as plain words, bn254_threshold.h; fr_from_u32 is reached
// through the Fr hook, op 6.)
BN_DEV Fr fr_from_u32(uint32_t x) {
  Fr a = fr_zero();
  a.w[0] = x;
  return fr_to_mont(a);
}
BN_DEV Fr fr_from_be(const uint8_t* p) {
  Fr a;
  scalar_from_be(a.w, p, true);
  return fr_to_mont(a);
}
// Montgomery form -> plain words (what g1_mul_glv_full takes) and 32 big-endian bytes
BN_DEV void fr_to_words(uint32_t* k, const Fr& a) {
  const Fr p = fr_from_mont(a);
  for (int i = 0; i < 8; ++i) k[i] = p.w[i];
}
BN_DEV void fr_to_be(uint8_t* p, const Fr& a) {
  uint32_t k[8];
  fr_to_words(k, a);
  u256_to_be(p, k);
}
// a^-1 = a^(r - 2) for a != 0 (zero maps to zero), bit by bit from the top: 253 squarings and one product per set bit of r - 2.  The low
// word of r is 0xf0000001, so r - 2 borrows nothing.
BN_DEV Fr fr_inv(const Fr& a) {
  Fr acc = fr_one();
  for (int bit = 253; bit >= 0; --bit) {
    acc = fr_mul(acc, acc);
    const uint32_t word = C_ORDER_R[bit >> 5] - (bit < 32 ? 2u : 0u);
    if ((word >> (bit & 31)) & 1u) acc = fr_mul(acc, a);
  }
  return acc;
}

}  // namespace bn254
