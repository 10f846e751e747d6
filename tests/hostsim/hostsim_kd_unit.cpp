// hostsim_kd_unit — TEST INFRASTRUCTURE ONLY.
//
// Host compilation (pair layout, both lane roles in sequence) of the keyed Miller loop on UNIT LINES (bn254_pairing.h:
// miller_loop_keyed_unit, the body of k_miller_verify_keyed_unit_pair; bn254_field.h: fp12_mul_unit_line) beside miller_loop_keyed.  Built
// plain and with -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb / value bound) by tests/test_kd_unit_lines.py.
#include <cstdint>
#include <cstring>

#define BN_SPLIT_FP2 1
#define BN_COUNT_FP_MUL 1
extern "C" { unsigned long long bn_fp_mul_counter = 0; unsigned long long bn_fp_dual_counter = 0; }
#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_pairing.h"

using namespace bn254;

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}
static bool all_zero(const uint8_t* b, int n) { uint8_t o = 0; for (int i = 0; i < n; ++i) o |= b[i]; return o == 0; }
static void load_g1(G1Affine& p, const uint8_t* b) { p.inf = all_zero(b, 64); p.x = fp_from_be32(b); p.y = fp_from_be32(b + 32); if (p.inf) { p.x = fp_load_const(C_G1_GEN[0]); p.y = fp_load_const(C_G1_GEN[1]); } }
static void load_g2(G2Affine& q, const uint8_t* b) {
  q.inf = all_zero(b, 128);
  if (q.inf) { q.x = fp2_load_const(C_G2_GEN[0]); q.y = fp2_load_const(C_G2_GEN[1]); return; }
  q.x.c[0] = fp_from_be32(b); q.x.c[1] = fp_from_be32(b + 32); q.y.c[0] = fp_from_be32(b + 64); q.y.c[1] = fp_from_be32(b + 96);
}
static void put_fp2(int32_t* w, const Fp2& x) {
  for (int r = 0; r < 2; ++r) for (int k = 0; k < BN_LIMBS; ++k) w[r * BN_LIMBS + k] = x.c[r].v[k];
}
static Fp2 canon2(const Fp2& x) { Fp2 r; for (int k = 0; k < 2; ++k) r.c[k] = fp_canon(x.c[k]); return r; }

typedef int32_t PlainTab[BN_N_FIXED_LINES][2][2][BN_LIMBS];

extern "C" {

// the first digit of the loop (the peeled step treats it generally; the test reports it)
int hu_first_digit(void) { return C_ATE_NAF[0]; }
// miller_loop_keyed and miller_loop_keyed_unit on one tuple (an all-zero h64 / sig64 = the identity: that pair is skipped; key_inf: the key
// is refused or the identity, pair A is skipped and the table is the generator's, as the device builds it): both values canonicalised
// coefficient by coefficient into plain108 / unit108 (12 x 9 words).  Returns 0, 249 = the table could not be built.
// counts (may be null): {keyed dual, keyed single, unit dual, unit single} products per LANE (both roles run here in sequence: totals / 2)
int hu_miller_both(const uint8_t* h64, const uint8_t* sig64, const uint8_t* pk128, int key_inf, int32_t* plain108, int32_t* unit108, unsigned long long* counts) {
  G1Affine h, sig;
  G2Affine pk;
  load_g1(h, h64); load_g1(sig, sig64); load_g2(pk, pk128);
  if (key_inf || pk.inf) { pk.x = fp2_load_const(C_G2_GEN[0]); pk.y = fp2_load_const(C_G2_GEN[1]); pk.inf = false; key_inf = 1; }
  static PlainTab tab;
  // the key's plain rows (g2_line_table + fp_canon: what registration and the key dedup store)
  if (!g2_line_table(pk, [&](int idx, const KeyLine& kl) { put_fp2(&tab[idx][0][0][0], canon2(kl.c0)); put_fp2(&tab[idx][1][0][0], canon2(kl.c1)); })) return 249;
  Fp12 f, g;
  unsigned long long m0 = bn_fp_mul_counter, d0 = bn_fp_dual_counter;
  miller_loop_keyed(f, h, key_inf != 0, tab, sig);
  if (counts) { counts[0] = (bn_fp_dual_counter - d0) / 2; counts[1] = ((bn_fp_mul_counter - m0) - (bn_fp_dual_counter - d0)) / 2; }
  m0 = bn_fp_mul_counter; d0 = bn_fp_dual_counter;
  miller_loop_keyed_unit(g, h, key_inf != 0, &tab[0][0][0][0], 0, sig);
  if (counts) { counts[2] = (bn_fp_dual_counter - d0) / 2; counts[3] = ((bn_fp_mul_counter - m0) - (bn_fp_dual_counter - d0)) / 2; }
  const Fp2* a[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  const Fp2* b[6] = {&g.c0.c0, &g.c0.c1, &g.c0.c2, &g.c1.c0, &g.c1.c1, &g.c1.c2};
  for (int k = 0; k < 6; ++k) { put_fp2(plain108 + k * 2 * BN_LIMBS, canon2(*a[k])); put_fp2(unit108 + k * 2 * BN_LIMBS, canon2(*b[k])); }
  return 0;
}

}  // extern "C"
