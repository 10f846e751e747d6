// hostsim_bitmap_rand — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the G1 side of the randomised signer-bitmap call (bn254_amd/csrc/bn254_bitmap_rand.h: bucket numbering, the byte of
// a bitmap, the keys of a window that carry a table pair, the fold of a window's byte buckets as k_bmr_fold runs it — every phase, lane
// after lane — and the places of the table pairs), in the pair layout of Fq2 and, with -DBM_ONE_LANE, the one-lane layout; built plain and
// with -DBN_TRACK_BOUNDS by tests/test_verify_keyed_bitmap_randomized.py.  A bucket's sum is formed with the complete addition the
// segmented sums use (jac_add), entry after entry.
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

using namespace bn254;

#include "../../bn254_amd/csrc/bn254_bitmap_rand.h"

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}
static void fp_to_be32(uint8_t* b, const Fp& a) {
  U256 x = fp_to_u256(a);
  for (int i = 0; i < 8; ++i) { b[28 - 4 * i] = (uint8_t)(x.w[i] >> 24); b[29 - 4 * i] = (uint8_t)(x.w[i] >> 16); b[30 - 4 * i] = (uint8_t)(x.w[i] >> 8); b[31 - 4 * i] = (uint8_t)x.w[i]; }
}
static void g1_from_bytes(G1Affine& p, const uint8_t* b) {
  uint8_t o = 0;
  for (int i = 0; i < 64; ++i) o |= b[i];
  p.inf = o == 0;
  p.x = fp_from_be32(b); p.y = fp_from_be32(b + 32);
}
static void g1_to_bytes(uint8_t* out, const G1Jac& j) {
  G1Affine a;
  jac_to_affine(a, j);
  if (a.inf) { memset(out, 0, 64); return; }
  fp_to_be32(out, a.x); fp_to_be32(out + 32, a.y);
}

extern "C" {

uint64_t hbr_bucket(uint64_t g, uint32_t w, uint32_t v, uint32_t n_keys) { return bmr_bucket(g, w, v, n_keys); }
uint64_t hbr_sig_bucket(uint64_t g, uint32_t n_keys) { return bmr_sig_bucket(g, n_keys); }
uint32_t hbr_byte(const uint32_t* row, size_t bm_words, uint32_t w) { return bmr_byte(row, bm_words, w); }
uint32_t hbr_window_keys(uint32_t w, uint32_t n_keys, const uint8_t* key_st, const uint8_t* key_inf) { return bmr_window_keys(w, n_keys, key_st, key_inf); }
uint32_t hbr_pair_rank(uint32_t mask, uint32_t b) { return bmr_pair_rank(mask, b); }

// One (group, window): n entries (64-byte affine points, zeros = the identity) with their bitmap rows; entry i goes into the bucket of byte
// w of its row (0: nowhere).  The buckets are summed, folded, and the table pairs of the keys in `mask` written in rank order: pair_key
// (8 w + b) and pair_point (zeros = a sum that came out as the identity).  all_t = the eight key sums whatever the mask.  Returns the
// number of pairs.
int hbr_window(size_t n, const uint8_t* pts, const uint32_t* rows, size_t bm_words, uint32_t w, uint32_t mask, uint32_t* pair_key, uint8_t* pair_point,
               uint8_t* all_t) {
  std::vector<BmrSlot> B(256), R(128), T(8);
  for (auto& s : B) jac_set_identity(s.v);
  for (auto& s : R) jac_set_identity(s.v);
  for (auto& s : T) jac_set_identity(s.v);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t v = bmr_byte(rows + i * bm_words, bm_words, w);
    if (v == 0) continue;
    G1Affine p;
    g1_from_bytes(p, pts + 64 * i);
    G1Jac j;
    jac_from_affine(j, p);
    jac_add(B[v].v, B[v].v, j);
  }
  for (int phase = 0; phase < BMR_FOLD_PHASES; ++phase)
    for (unsigned t = 0; t < 256; ++t) bmr_fold_phase(B.data(), R.data(), T.data(), phase, t);
  int pairs = 0;
  for (uint32_t b = 0; b < 8; ++b) {
    g1_to_bytes(all_t + 64 * b, T[b].v);
    if (!((mask >> b) & 1u)) continue;
    const uint32_t at = bmr_pair_rank(mask, b);
    pair_key[at] = 8u * w + b;
    g1_to_bytes(pair_point + 64 * at, T[b].v);
    ++pairs;
  }
  return pairs;
}

}  // extern "C"
