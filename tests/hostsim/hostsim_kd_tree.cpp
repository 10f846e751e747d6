// hostsim_kd_tree — TEST INFRASTRUCTURE ONLY.
//
// Host compilation (pair layout, both lane roles in sequence) of the scaling pass of the key dedup's table builder: kd_scale_tree
// (bn254_amd/csrc/bn254_keydedup.h — one inversion per key, the product tree k_kd_scale runs on the device) against kd_scale_line (one
// inversion per line) on the raw lines of the builder's level program, and against g2_line_table + fp_canon.  Built plain and with
// -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb / value bound) by tests/test_kd_scale_tree.py.
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

// the 87 x (c0, c1) x (re, im) x 9 words of key pk128 (on the curve, not the identity) three ways: `ref` g2_line_table + fp_canon, `line`
// the builder's raw lines through kd_scale_line, `tree` the same raw lines through kd_scale_tree.  Returns 0, 1 if a line has c2 = 0
// (then only ref and line are meaningful), 3 if the point is not on the curve, 4 on a wrong line count.
int kt_tables(const uint8_t* pk128, int32_t* ref, int32_t* line, int32_t* tree) {
  G2Affine q;
  q.inf = false;
  q.x.c[0] = fp_from_be32(pk128); q.x.c[1] = fp_from_be32(pk128 + 32); q.y.c[0] = fp_from_be32(pk128 + 64); q.y.c[1] = fp_from_be32(pk128 + 96);
  if (!g2_on_curve(q)) return 3;
  const int W = 4 * BN_LIMBS;
  auto put = [&](int32_t* out, int idx, const Fp2& r0, const Fp2& r1) {
    const Fp c[4] = {r0.c[0], r0.c[1], r1.c[0], r1.c[1]};
    for (int e = 0; e < 4; ++e)
      for (int k = 0; k < BN_LIMBS; ++k) out[idx * W + e * BN_LIMBS + k] = c[e].v[k];
  };
  g2_line_table(q, [&](int idx, const KeyLine& kl) {
    Fp2 a, b;
    for (int k = 0; k < 2; ++k) { a.c[k] = fp_canon(kl.c0.c[k]); b.c[k] = fp_canon(kl.c1.c[k]); }
    put(ref, idx, a, b);
  });
  static Fp2 c0[BN_N_FIXED_LINES], c1[BN_N_FIXED_LINES], c2[BN_N_FIXED_LINES], r0[BN_N_FIXED_LINES], r1[BN_N_FIXED_LINES];
  int lines = 0;
  const bool degenerate = kd_builder_model(q, [&](int idx, const Fp2& a, const Fp2& b, const Fp2& c) {
    c0[idx] = a; c1[idx] = b; c2[idx] = c;
    Fp2 s0, s1;
    kd_scale_line(a, b, c, s0, s1);
    put(line, idx, s0, s1);
    ++lines;
  });
  if (lines != BN_N_FIXED_LINES) return 4;
  kd_scale_tree(c0, c1, c2, r0, r1);           // with a zero c2 too: must terminate (and, under the tracker, stay within bounds)
  for (int idx = 0; idx < BN_N_FIXED_LINES; ++idx) put(tree, idx, r0[idx], r1[idx]);
  return degenerate ? 1 : 0;
}

}  // extern "C"
