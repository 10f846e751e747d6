// hostsim_aggd_rand — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the G1 side of the randomised keyed aggregate verify (bn254_aggrand.h, as k_aggr_scale / k_aggr_sum use it) and of
// its group checks: r_i from rand_scalar with i = the aggregate's index, the entries scaled (a group with one aggregate: r = 1), summed per
// (group, key) bucket with the signatures in bucket K, and per group the slot loop over the non-empty key buckets' table pairs and
// (S_g, -G2) (miller_loop_tables on tables built as registration builds them), then the exact final exponentiation.
// Built plain and with -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb / value bound) by
// tests/test_aggregate_distinct_keyed_randomized.py.
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
#include "../../bn254_amd/csrc/bn254_hash.h"

using namespace bn254;

#include "../../bn254_amd/csrc/bn254_aggrand.h"

typedef int32_t KeyTab[BN_N_FIXED_LINES][2][2][BN_LIMBS];

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}
static void fp_to_be32(uint8_t* b, const Fp& a) {
  const U256 x = fp_to_u256(a);
  for (int i = 0; i < 8; ++i) for (int k = 0; k < 4; ++k) b[4 * i + k] = (uint8_t)(x.w[7 - i] >> (24 - 8 * k));
}
static bool all_zero(const uint8_t* b, int n) { uint8_t o = 0; for (int i = 0; i < n; ++i) o |= b[i]; return o == 0; }
static void load_g1(G1Affine& p, const uint8_t* b) {
  p.inf = all_zero(b, 64);
  p.x = fp_from_be32(b); p.y = fp_from_be32(b + 32);
}
static void store_g1(uint8_t* b, const G1Jac& j) {
  G1Affine a;
  jac_to_affine(a, j);
  if (a.inf) { memset(b, 0, 64); return; }
  fp_to_be32(b, a.x); fp_to_be32(b + 32, a.y);
}
static void seed_words(uint32_t* w, const uint8_t* seed32) {
  for (int j = 0; j < 8; ++j) w[j] = ((uint32_t)seed32[4 * j] << 24) | ((uint32_t)seed32[4 * j + 1] << 16) | ((uint32_t)seed32[4 * j + 2] << 8) | seed32[4 * j + 3];
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

extern "C" {

// r_i * p (bn254_aggrand.h: aggr_scale), affine, 64 big-endian bytes (all zero: the identity)
void har_scale(const uint8_t* p64, const uint8_t* seed32, uint64_t i, int mode, int one, uint8_t* out64) {
  uint32_t w[8];
  seed_words(w, seed32);
  G1Affine p;
  load_g1(p, p64);
  G1Jac acc;
  aggr_scale(acc, p, w, i, mode, one != 0);
  store_g1(out64, acc);
}

// n aggregates, aggregate i = pairs [agg_off[i], agg_off[i+1]) of (H = hs + 64 j, key key_idx[j] < n_keys) and sigma = sigs + 64 i, all at
// the check.  Out: the bucket sums (n_groups (n_keys + 1) points of 64 bytes; bucket (g, n_keys) = S_g), per group its verdict (0 / 9, 255
// for a group without aggregates) and in *table_pairs the table pairs of all group checks.  Returns 0, or 251 if a key's table failed.
int har_groups(size_t n_keys, const uint8_t* pks, size_t m, const uint8_t* hs, const uint32_t* key_idx, size_t n, const uint64_t* agg_off, const uint8_t* sigs,
               const uint8_t* seed32, int mode, uint64_t group_pairs, uint8_t* buckets, uint8_t* verdict, uint64_t* table_pairs) {
  const uint32_t K = (uint32_t)n_keys;
  const uint64_t G = group_pairs > n_keys ? group_pairs : n_keys, ng = m / G + 1, n_b = ng * (K + 1);
  std::vector<KeyTab> tabs(K + 1);
  std::vector<bool> inf(K + 1);
  for (uint32_t k = 0; k < K; ++k) {
    bool i_;
    if (!register_key(pks + 128 * k, tabs[k], i_)) return 251;
    inf[k] = i_;
  }
  for (int idx = 0; idx < BN_N_FIXED_LINES; ++idx)
    for (int w = 0; w < 4 * BN_LIMBS; ++w) (&tabs[K][idx][0][0][0])[w] = neg_g2_key_line_word(idx, w);
  uint32_t sw[8];
  seed_words(sw, seed32);
  std::vector<uint32_t> nagg(ng, 0);
  for (size_t i = 0; i < n; ++i) ++nagg[aggr_group(agg_off[i], G)];
  std::vector<G1Jac> sum(n_b);
  std::vector<uint64_t> cnt(n_b, 0);
  for (auto& s : sum) jac_set_identity(s);
  auto add = [&](uint64_t b, const uint8_t* p64, size_t i, bool one) {
    G1Affine p;
    load_g1(p, p64);
    G1Jac a;
    aggr_scale(a, p, sw, i, mode, one);
    jac_add(sum[b], sum[b], a);
    ++cnt[b];
  };
  for (size_t i = 0; i < n; ++i) {
    const uint64_t g = aggr_group(agg_off[i], G);
    const bool one = nagg[g] == 1;
    for (uint64_t j = agg_off[i]; j < agg_off[i + 1]; ++j)
      if (!inf[key_idx[j]]) add(aggr_bucket(g, key_idx[j], K), hs + 64 * j, i, one);
    add(aggr_bucket(g, K, K), sigs + 64 * i, i, one);
  }
  for (uint64_t b = 0; b < n_b; ++b) store_g1(buckets + 64 * b, sum[b]);
  *table_pairs = 0;
  for (uint64_t g = 0; g < ng; ++g) {
    if (!nagg[g]) { verdict[g] = 255; continue; }
    Fp12 acc, f;
    fp12_set_one(acc);
    for (uint32_t key = 0; key <= K; ++key) {
      const uint64_t b = aggr_bucket(g, key, K);
      if (key < K && !cnt[b]) continue;
      G1Affine p;
      jac_to_affine(p, sum[b]);
      miller_loop_tables<1>(f, p, p.inf, tabs[key], p, true, tabs[key]);
      fp12_mul(acc, acc, f);
      ++*table_pairs;
    }
    fe_machine_exact(acc);
    verdict[g] = fp12_is_one(acc) ? 0 : 9;
  }
  return 0;
}

}  // extern "C"
