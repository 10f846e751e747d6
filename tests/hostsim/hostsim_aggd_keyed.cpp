// hostsim_aggd_keyed — TEST INFRASTRUCTURE ONLY.
//
// Host compilation (pair layout, both lane roles in sequence) of the slot loop of the aggregates over distinct messages against registered
// keys (bn254_aggkeyed.hip: k_aggd_keyed_pair): every key tabulated as registration stores it (g2_line_table + fp_canon, bn254_rand.hip:
// k_register_keys), -G2's lines in the same format (neg_g2_key_line_word: k_neg_g2_key_lines), the k + 1 table pairs of one aggregate taken
// `width` per slot through miller_loop_tables, the slot values multiplied (the segmented product), then the exact final exponentiation.
// Built plain and with -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb / value bound) by tests/test_aggregate_distinct_keyed.py.
#include <cstdint>
#include <cstring>
#include <vector>

#define BN_SPLIT_FP2 1
#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_pairing.h"

using namespace bn254;

typedef int32_t KeyTab[BN_N_FIXED_LINES][2][2][BN_LIMBS];

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}
static bool all_zero(const uint8_t* b, int n) { uint8_t o = 0; for (int i = 0; i < n; ++i) o |= b[i]; return o == 0; }
static void load_g1(G1Affine& p, const uint8_t* b) {
  p.inf = all_zero(b, 64);
  p.x = fp_from_be32(b); p.y = fp_from_be32(b + 32);
  if (p.inf) { p.x = fp_load_const(C_G1_GEN[0]); p.y = fp_load_const(C_G1_GEN[1]); }
}
// registration: the key's table (the generator's for the identity, as k_register_keys walks it) and its identity flag
static bool register_key(const uint8_t* pk128, KeyTab& tab, bool& inf) {
  G2Affine q;
  inf = all_zero(pk128, 128);
  if (inf) { q.x = fp2_load_const(C_G2_GEN[0]); q.y = fp2_load_const(C_G2_GEN[1]); }
  else { q.x.c[0] = fp_from_be32(pk128); q.x.c[1] = fp_from_be32(pk128 + 32); q.y.c[0] = fp_from_be32(pk128 + 64); q.y.c[1] = fp_from_be32(pk128 + 96); }
  q.inf = false;
  return g2_line_table(q, [&](int idx, const KeyLine& kl) {
    const Fp2* c[2] = {&kl.c0, &kl.c1};
    for (int e = 0; e < 2; ++e)
      for (int r = 0; r < 2; ++r) { const Fp x = fp_canon(c[e]->c[r]); for (int k = 0; k < BN_LIMBS; ++k) tab[idx][e][r][k] = x.v[k]; }
  });
}
static void neg_g2_table(KeyTab& tab) {
  for (int idx = 0; idx < BN_N_FIXED_LINES; ++idx)
    for (int w = 0; w < 4 * BN_LIMBS; ++w) (&tab[idx][0][0][0])[w] = neg_g2_key_line_word(idx, w);
}
static bool fp12_same(const Fp12& f, const Fp12& g) {
  const Fp2* a[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  const Fp2* b[6] = {&g.c0.c0, &g.c0.c1, &g.c0.c2, &g.c1.c0, &g.c1.c1, &g.c1.c2};
  for (int k = 0; k < 6; ++k) if (!fp2_eq(*a[k], *b[k])) return false;
  return true;
}

extern "C" {

// -G2's 87 lines as registration appends them behind the keys: 87 x 2 x 2 x 9 words
void hak_neg_g2_table(int32_t* out) {
  static KeyTab tab;
  neg_g2_table(tab);
  memcpy(out, tab, sizeof tab);
}

// One aggregate: k pairs (H(m_j) = h64s + 64 j, pk_j = pk128s + 128 j; all-zero bytes = the identity) and sigma, through the slot loop of
// `width` table pairs per slot.  Returns 0 / 9 (the product after the final exponentiation is / is not one), 251 if a key's table could
// not be built, 252 if the value differs from the product of per-pair miller_loop_keyed values (each pair alone, the other side skipped).
int hak_aggregate(int k, const uint8_t* h64s, const uint8_t* pk128s, const uint8_t* sig64, int width) {
  std::vector<KeyTab> tabs(k + 1);
  std::vector<bool> skip(k + 1);
  std::vector<G1Affine> pts(k + 1);
  for (int j = 0; j < k; ++j) {
    bool inf;
    if (!register_key(pk128s + 128 * j, tabs[j], inf)) return 251;
    load_g1(pts[j], h64s + 64 * j);
    skip[j] = inf || pts[j].inf;
  }
  neg_g2_table(tabs[k]);                        // table pair k: (sigma, -G2)
  load_g1(pts[k], sig64);
  skip[k] = pts[k].inf;
  // the slot loop: table pairs W s .. W s + W - 1, a pair past k pads (skipped, -G2's table, sigma's point — as the kernel loads it)
  Fp12 acc, f;
  fp12_set_one(acc);
  for (int t0 = 0; t0 <= k; t0 += width) {
    const int t1 = t0 + 1 <= k ? t0 + 1 : k;
    const bool skip1 = t0 + 1 > k || skip[t1];
    if (width == 2) miller_loop_tables<2>(f, pts[t0], skip[t0], tabs[t0], pts[t1], skip1, tabs[t1]);
    else miller_loop_tables<1>(f, pts[t0], skip[t0], tabs[t0], pts[t0], true, tabs[t0]);
    fp12_mul(acc, acc, f);
  }
  // per pair, the keyed verify's loop with the other side skipped
  Fp12 ref;
  fp12_set_one(ref);
  G1Affine none = pts[k];
  none.inf = true;
  for (int j = 0; j <= k; ++j) {
    if (j < k) miller_loop_keyed(f, pts[j], skip[j], tabs[j], none);
    else miller_loop_keyed(f, none, true, tabs[0 < k ? 0 : k], pts[k]);
    fp12_mul(ref, ref, f);
  }
  fe_machine_exact(acc);
  fe_machine_exact(ref);
  if (!fp12_same(acc, ref)) return 252;
  return fp12_is_one(acc) ? 0 : 9;
}

}  // extern "C"
