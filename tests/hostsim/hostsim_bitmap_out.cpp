// hostsim_bitmap_out — TEST INFRASTRUCTURE ONLY.
//
// Host compilation (pair layout of Fq2; -DBM_ONE_LANE: the one-lane layout) of the per-item bodies of bn254_amd/csrc/bn254_bitmap_out.h —
// the very functions k_bmo_emit, k_bmo_settle, k_bmw_build and k_bmw_sum run — behind a registered set, its bad-bit vector and its subset
// tables built by bn254_bitmap.h as the first bitmap call builds them, as a stand-alone program: the kernels' grids are emulated as a loop
// over blocks of 64 lanes with the kernels' own bound check.  Built plain, with -fsanitize=address,undefined and with -DBN_TRACK_BOUNDS by
// tests/test_bitmap_out_cases.py, which compares what it writes with the oracle and with Python integers.  Every buffer has its exact size.
//
//   hostsim_bitmap_out IN OUT
//   IN : u64 n_keys | u64 n | u64 bm_words | u64 tables (0: key by key) — little-endian —
//        n_keys * 128 key encodings | n_keys registration statuses | n_keys u64 weights |
//        n * bm_words u32 bitmap words | n * 64 H(m) | n hash statuses | n decode statuses of sigma | n final statuses of the verify
//   OUT: n * 128 keys of call A | n statuses of call A | n * 64 hashes of call B | n * 128 keys of call B (both behind the settle) |
//        n u64 weights | n statuses of the weight call
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
#include "../../bn254_amd/csrc/bn254_bitmap_out.h"

using namespace bn254;

static const size_t WAVE = 64;

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}
static bool all_zero(const uint8_t* b, int n) { uint8_t o = 0; for (int i = 0; i < n; ++i) o |= b[i]; return o == 0; }
#if defined(BN_SPLIT_FP2)
static const Fp& re_of(const Fp2& a) { return a.c[0]; }
static const Fp& im_of(const Fp2& a) { return a.c[1]; }
#else
static const Fp& re_of(const Fp2& a) { return a.c0; }
static const Fp& im_of(const Fp2& a) { return a.c1; }
#endif

template <class T> static T* alloc(size_t count) {
  T* p = (T*)malloc(count ? count * sizeof(T) : 1);
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}
static void need(bool ok) { if (!ok) { fprintf(stderr, "short input\n"); exit(2); } }

// what the sum kernels leave of entry i, then k_bmo_emit: the key under the entry's status (sigma's decode status, rule 2 behind it), H(m)
// under that and the hash status
struct Entry { G2Affine pk; uint8_t st; };
static void sum_entry(Entry& e, const uint32_t* row, size_t bm_words, const BmKeys& K, const int32_t* rec, const uint8_t* rec_inf, uint8_t decode_st) {
  G2Jac acc;
  if (rec) bm_sum_tables(acc, row, bm_words, true, K, rec, rec_inf);
  else bm_sum_keys(acc, row, bm_words, true, K);
  bm_sum_to_key(e.pk, acc);
  e.st = decode_st != ST_OK ? decode_st : bm_rule2_status(row, bm_words, K);
}
static void emit_key(uint8_t* out128, const Entry& e) { bmo_emit_key(out128, re_of(e.pk.x), im_of(e.pk.x), re_of(e.pk.y), im_of(e.pk.y), e.pk.inf, e.st); }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t hdr[4];
  need(fread(hdr, 8, 4, f) == 4);
  const uint32_t n_keys = (uint32_t)hdr[0];
  const size_t n = (size_t)hdr[1], bm_words = (size_t)hdr[2];
  const bool tables = hdr[3] != 0;
  uint8_t* pk = alloc<uint8_t>(128 * (size_t)n_keys);
  uint8_t* key_st = alloc<uint8_t>(n_keys);
  uint64_t* weights = alloc<uint64_t>(n_keys);
  uint32_t* bits = alloc<uint32_t>(n * bm_words);
  uint8_t* hm = alloc<uint8_t>(64 * n);
  uint8_t *hash_st = alloc<uint8_t>(n), *decode_st = alloc<uint8_t>(n), *final_st = alloc<uint8_t>(n);
  if (n_keys) need(fread(pk, 128, n_keys, f) == n_keys && fread(key_st, 1, n_keys, f) == n_keys && fread(weights, 8, n_keys, f) == n_keys);
  if (n && bm_words) need(fread(bits, 4, n * bm_words, f) == n * bm_words);
  if (n) need(fread(hm, 64, n, f) == n && fread(hash_st, 1, n, f) == n && fread(decode_st, 1, n, f) == n && fread(final_st, 1, n, f) == n);
  fclose(f);

  // the registered set as k_register_keys leaves it (the generator's coordinates for a refused or identity key), the bad-bit vector and the
  // subset tables as bm_prepare builds them, the weight tables as bn254_ctx_set_key_weights builds them
  const uint32_t n_words = (n_keys + 31) / 32, n_windows = (n_keys + 7) / 8;
  const size_t entries = (size_t)n_windows * 256;
  int32_t* xy = alloc<int32_t>((size_t)n_keys * BM_KEY_WORDS);
  uint8_t* key_inf = alloc<uint8_t>(n_keys);
  for (uint32_t j = 0; j < n_keys; ++j) {
    const uint8_t* b = pk + 128 * (size_t)j;
    key_inf[j] = key_st[j] == 0 && all_zero(b, 128);
    Fp c[4];
    if (key_st[j] != 0 || key_inf[j]) { c[0] = fp_load_const(C_G2_GEN[0][0]); c[1] = fp_load_const(C_G2_GEN[0][1]); c[2] = fp_load_const(C_G2_GEN[1][0]); c[3] = fp_load_const(C_G2_GEN[1][1]); }
    else for (int e = 0; e < 4; ++e) c[e] = fp_from_be32(b + 32 * e);
    for (int e = 0; e < 4; ++e) for (int k = 0; k < BN_LIMBS; ++k) xy[((size_t)j * 4 + e) * BN_LIMBS + k] = c[e].v[k];
  }
  uint32_t* bad = alloc<uint32_t>(n_words);
  for (uint32_t w = 0; w < n_words; ++w) bad[w] = bm_bad_word(key_st, n_keys, w);
  const BmKeys K = {xy, key_st, key_inf, bad, n_keys};
  int32_t* rec = nullptr;
  uint8_t* rec_inf = nullptr;
  if (tables && n_keys) {
    rec = alloc<int32_t>(entries * BM_REC_WORDS);
    rec_inf = alloc<uint8_t>(entries);
    memset(rec, 0, entries * BM_REC_WORDS * sizeof(int32_t));     // the two pad words of a half record are never written
    const BmTable T = {rec, rec_inf};
    for (size_t j = 0; j < entries; ++j) {
      G2Affine a;
      bm_subset_entry(a, K, (uint32_t)(j >> 8), (uint32_t)(j & 255u), true);
      bm_store_entry(T, j, a);
      T.inf[j] = a.inf;
    }
  }
  uint64_t* wtab = alloc<uint64_t>(entries);
  for (size_t b = 0; b < (entries + WAVE - 1) / WAVE; ++b)
    for (size_t t = 0; t < WAVE; ++t) {                            // k_bmw_build
      const size_t j = b * WAVE + t;
      if (j < entries) wtab[j] = bmw_subset_entry(weights, n_keys, (uint32_t)(j >> 8), (uint32_t)(j & 255u));
    }

  uint32_t* keys_a = alloc<uint32_t>(32 * n);
  uint32_t* keys_b = alloc<uint32_t>(32 * n);
  uint32_t* hashes_b = alloc<uint32_t>(16 * n);
  uint64_t* weight = alloc<uint64_t>(n);
  uint8_t *st_a = alloc<uint8_t>(n), *st_w = alloc<uint8_t>(n);
  const size_t blocks = (n + WAVE - 1) / WAVE;
  for (size_t b = 0; b < blocks; ++b)
    for (size_t t = 0; t < WAVE; ++t) {
      const size_t i = b * WAVE + t;
      if (i >= n) continue;
      const uint32_t* row = bits + i * bm_words;
      Entry e;
      // call A: the decode plane cleared, the sum, k_bmo_emit with the status array
      sum_entry(e, row, bm_words, K, rec, rec_inf, ST_OK);
      emit_key((uint8_t*)keys_a + 128 * i, e);
      st_a[i] = e.st;
      // call B: sigma's decode status in front, k_bmo_emit into both outputs, then k_bmo_settle under the verify's final status
      sum_entry(e, row, bm_words, K, rec, rec_inf, decode_st[i]);
      emit_key((uint8_t*)keys_b + 128 * i, e);
      bmo_emit_hash((uint8_t*)hashes_b + 64 * i, fp_from_be32(hm + 64 * i), fp_from_be32(hm + 64 * i + 32), false, e.st != ST_OK ? e.st : hash_st[i]);
    }
  for (size_t b = 0; b < blocks; ++b)
    for (size_t t = 0; t < WAVE; ++t) {
      const size_t i = b * WAVE + t;
      if (i >= n) continue;
      bmo_settle_item(final_st[i], (uint8_t*)hashes_b + 64 * i, (uint8_t*)keys_b + 128 * i);
      bmw_item(bits + i * bm_words, bm_words, K, wtab, weight[i], st_w[i]);   // k_bmw_sum
    }
#if defined(BN_TRACK_BOUNDS)
  if (::bn_bound_failed) { fprintf(stderr, "a limb / value bound was violated\n"); return 3; }
#endif
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  bool ok = true;
  if (n) ok = fwrite(keys_a, 128, n, f) == n && fwrite(st_a, 1, n, f) == n && fwrite(hashes_b, 64, n, f) == n && fwrite(keys_b, 128, n, f) == n &&
              fwrite(weight, 8, n, f) == n && fwrite(st_w, 1, n, f) == n;
  ok = fclose(f) == 0 && ok;
  free(pk); free(key_st); free(weights); free(bits); free(hm); free(hash_st); free(decode_st); free(final_st); free(xy); free(key_inf); free(bad);
  free(rec); free(rec_inf); free(wtab); free(keys_a); free(keys_b); free(hashes_b); free(weight); free(st_a); free(st_w);
  if (!ok) { fprintf(stderr, "short output\n"); return 2; }
  printf("hostsim_bitmap_out ok: %zu rows over %u keys\n", n, n_keys);
  return 0;
}
