// hostsim_bitmap — TEST INFRASTRUCTURE ONLY.
//
// Host compilation (pair layout, both lane roles in sequence; -DBM_ONE_LANE: the one-lane layout) of the aggregate key of a signer bitmap
// over registered keys (bn254_amd/csrc/bn254_bitmap.h: the table builder, the bitmap walk with and without tables, the rule-2 scan) — the
// very functions k_bm_build_tables, k_bm_sum_pair and k_bm_sum run.  Built plain and with -DBN_TRACK_BOUNDS (the interval tracker aborts on
// a violated limb / value bound, and on a table entry outside the stored-word contract) by tests/test_verify_keyed_bitmap.py.
#include <cstdint>
#include <cstring>
#include <vector>

#if !defined(BM_ONE_LANE)
#define BN_SPLIT_FP2 1
#endif
#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_pairing.h"
#include "../../bn254_amd/csrc/bn254_bitmap.h"

using namespace bn254;

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}
static void fp_to_be32(uint8_t* b, const Fp& a) {
  U256 x = fp_to_u256(a);
  for (int i = 0; i < 8; ++i) { b[28 - 4 * i] = (uint8_t)(x.w[i] >> 24); b[29 - 4 * i] = (uint8_t)(x.w[i] >> 16); b[30 - 4 * i] = (uint8_t)(x.w[i] >> 8); b[31 - 4 * i] = (uint8_t)x.w[i]; }
}
static bool all_zero(const uint8_t* b, int n) { uint8_t o = 0; for (int i = 0; i < n; ++i) o |= b[i]; return o == 0; }
#if defined(BN_SPLIT_FP2)
static const Fp& re_of(const Fp2& a) { return a.c[0]; }
static const Fp& im_of(const Fp2& a) { return a.c[1]; }
#else
static const Fp& re_of(const Fp2& a) { return a.c0; }
static const Fp& im_of(const Fp2& a) { return a.c1; }
#endif
static void g2_to_bytes(uint8_t* out128, const G2Affine& q) {
  if (q.inf) { memset(out128, 0, 128); return; }
  fp_to_be32(out128, re_of(q.x)); fp_to_be32(out128 + 32, im_of(q.x)); fp_to_be32(out128 + 64, re_of(q.y)); fp_to_be32(out128 + 96, im_of(q.y));
}

// the registered set as k_register_keys leaves it: key_xy (the generator's coordinates for a refused or identity key), key_st, key_inf —
// and what the first bitmap call builds from it: the bad-bit vector and the subset tables
static std::vector<int32_t> g_xy, g_rec;
static std::vector<uint8_t> g_st, g_inf, g_rec_inf;
static std::vector<uint32_t> g_bad;
static uint32_t g_n_keys = 0;
static BmKeys keys() { return BmKeys{g_xy.data(), g_st.data(), g_inf.data(), g_bad.data(), g_n_keys}; }

extern "C" {

// pk128s: n_keys uncompressed keys (all-zero = the identity); key_st: their registration statuses (non-zero = refused).  Builds everything.
void hb_register(uint32_t n_keys, const uint8_t* pk128s, const uint8_t* key_st) {
  g_n_keys = n_keys;
  g_xy.assign((size_t)n_keys * BM_KEY_WORDS + 1, 0); g_st.assign(n_keys + 1, 0); g_inf.assign(n_keys + 1, 0);
  for (uint32_t j = 0; j < n_keys; ++j) {
    const uint8_t* b = pk128s + 128 * (size_t)j;
    g_st[j] = key_st[j];
    g_inf[j] = key_st[j] == 0 && all_zero(b, 128);
    Fp c[4];
    if (g_st[j] != 0 || g_inf[j]) { c[0] = fp_load_const(C_G2_GEN[0][0]); c[1] = fp_load_const(C_G2_GEN[0][1]); c[2] = fp_load_const(C_G2_GEN[1][0]); c[3] = fp_load_const(C_G2_GEN[1][1]); }
    else for (int e = 0; e < 4; ++e) c[e] = fp_from_be32(b + 32 * e);
    for (int e = 0; e < 4; ++e) for (int k = 0; k < BN_LIMBS; ++k) g_xy[((size_t)j * 4 + e) * BN_LIMBS + k] = c[e].v[k];
  }
  const uint32_t n_words = (n_keys + 31) / 32, n_windows = (n_keys + 7) / 8;
  g_bad.assign(n_words + 1, 0);
  for (uint32_t w = 0; w < n_words; ++w) g_bad[w] = bm_bad_word(g_st.data(), n_keys, w);
  g_rec.assign((size_t)n_windows * 256 * BM_REC_WORDS + 1, 0); g_rec_inf.assign((size_t)n_windows * 256 + 1, 0);
  const BmKeys K = keys();
  const BmTable T = {g_rec.data(), g_rec_inf.data()};
  for (size_t j = 0; j < (size_t)n_windows * 256; ++j) {
    G2Affine a;
    bm_subset_entry(a, K, (uint32_t)(j >> 8), (uint32_t)(j & 255u), true);
    bm_store_entry(T, j, a);
    T.inf[j] = a.inf;
  }
}
// table entry window * 256 + mask as bytes (zeros = the identity)
void hb_table_entry(uint32_t window, uint32_t mask, uint8_t* out128) {
  G2Affine q;
  const size_t j = (size_t)window * 256 + mask;
  BmRecSrc{g_rec.data() + j * BM_REC_WORDS, g_rec_inf[j] != 0}(q);
  g2_to_bytes(out128, q);
}
// one tuple: the walk (tables != 0: over the subset tables, else key by key) and the rule-2 scan.  out128 = the aggregate key (zeros = the
// identity); *gen_under_inf = 1 iff an identity sum carries the generator's coordinates, as the verify kernels are handed it.  Returns the
// rule-2 status.
int hb_sum(const uint32_t* row, size_t bm_words, int tables, uint8_t* out128, int* gen_under_inf) {
  const BmKeys K = keys();
  G2Jac acc;
  if (tables) bm_sum_tables(acc, row, bm_words, true, K, g_rec.data(), g_rec_inf.data());
  else bm_sum_keys(acc, row, bm_words, true, K);
  G2Affine pk;
  bm_sum_to_key(pk, acc);
  if (gen_under_inf) *gen_under_inf = pk.inf && fp2_eq(pk.x, fp2_load_const(C_G2_GEN[0])) && fp2_eq(pk.y, fp2_load_const(C_G2_GEN[1]));
  g2_to_bytes(out128, pk);
  return bm_rule2_status(row, bm_words, K);
}
size_t hb_table_bytes_per_key(void) { return BM_TABLE_BYTES_PER_KEY; }

}  // extern "C"
