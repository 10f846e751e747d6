// hostsim_kd_builder — TEST INFRASTRUCTURE ONLY.
//
// Host compilation (pair layout, both lane roles in sequence) of the key-table builder of the exact verify's key dedup
// (bn254_amd/csrc/bn254_kdlines.h, run by k_kd_lines in bn254_keydedup.hip): the lane machine's level program on a host box per key, its
// raw lines through kd_scale_line, must give word for word the table of g2_line_table + fp_canon, and must flag a line with c2 = 0 exactly
// when g2_line_table does.  Built plain and with -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb / value bound) by
// tests/test_kd_builder.py.
#include <cstdint>
#include <cstring>

#define BN_SPLIT_FP2 1
#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_pairing.h"
#include "../../bn254_amd/csrc/bn254_keydedup.h"
#include "../../bn254_amd/csrc/bn254_nonet.h"
#include "../../bn254_amd/csrc/bn254_lmachine.h"
#include "../../bn254_amd/csrc/bn254_kdlines.h"

using namespace bn254;

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}

extern "C" {

// the 87 x (c0, c1) x (re, im) x 9 words of key pk128 (an on-curve, non-identity uncompressed G2 point) both ways: `ref` from g2_line_table +
// fp_canon, `kd` from the builder's level program + kd_scale_line.  Returns 0, or 1 if a line has c2 = 0 (both sides agree on that), 2 if
// they disagree on it, 3 if the point is not on the curve.  On 1 the tables are compared all the same: the zero line's entries are 0 / 0
// on both sides.
int kb_tables(const uint8_t* pk128, int32_t* ref, int32_t* kd) {
  G2Affine q;
  q.inf = false;
  q.x.c[0] = fp_from_be32(pk128); q.x.c[1] = fp_from_be32(pk128 + 32); q.y.c[0] = fp_from_be32(pk128 + 64); q.y.c[1] = fp_from_be32(pk128 + 96);
  if (!g2_on_curve(q)) return 3;
  const int W = 4 * BN_LIMBS;
  const bool ok = g2_line_table(q, [&](int idx, const KeyLine& kl) {
    const Fp c[4] = {fp_canon(kl.c0.c[0]), fp_canon(kl.c0.c[1]), fp_canon(kl.c1.c[0]), fp_canon(kl.c1.c[1])};
    for (int e = 0; e < 4; ++e)
      for (int k = 0; k < BN_LIMBS; ++k) ref[idx * W + e * BN_LIMBS + k] = c[e].v[k];
  });
  int lines = 0;
  const bool degenerate = kd_builder_model(q, [&](int idx, const Fp2& c0, const Fp2& c1, const Fp2& c2) {
    Fp2 r0, r1;
    kd_scale_line(c0, c1, c2, r0, r1);
    const Fp c[4] = {r0.c[0], r0.c[1], r1.c[0], r1.c[1]};
    for (int e = 0; e < 4; ++e)
      for (int k = 0; k < BN_LIMBS; ++k) kd[idx * W + e * BN_LIMBS + k] = c[e].v[k];
    ++lines;
  });
  if (lines != BN_N_FIXED_LINES) return 4;
  if (degenerate == ok) return 2;
  return degenerate ? 1 : 0;
}

// the raw lines (c0, c1, c2) of both walks, canonical: the builder's must equal kd_walk_raw_lines's as field elements (87 x 3 x 2 x 9 words)
int kb_raw(const uint8_t* pk128, int32_t* walk, int32_t* lm) {
  G2Affine q;
  q.inf = false;
  q.x.c[0] = fp_from_be32(pk128); q.x.c[1] = fp_from_be32(pk128 + 32); q.y.c[0] = fp_from_be32(pk128 + 64); q.y.c[1] = fp_from_be32(pk128 + 96);
  if (!g2_on_curve(q)) return 3;
  const int W = 6 * BN_LIMBS;
  auto put = [&](int32_t* out) {
    return [out, W](int idx, const Fp2& c0, const Fp2& c1, const Fp2& c2) {
      const Fp c[6] = {fp_canon(c0.c[0]), fp_canon(c0.c[1]), fp_canon(c1.c[0]), fp_canon(c1.c[1]), fp_canon(c2.c[0]), fp_canon(c2.c[1])};
      for (int e = 0; e < 6; ++e)
        for (int k = 0; k < BN_LIMBS; ++k) out[idx * W + e * BN_LIMBS + k] = c[e].v[k];
    };
  };
  const bool a = kd_walk_raw_lines(q, put(walk));
  const bool b = kd_builder_model(q, put(lm));
  return a == b ? 0 : 2;
}

}  // extern "C"
