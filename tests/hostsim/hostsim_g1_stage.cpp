// hostsim_g1_stage — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the per-item bodies behind BN254_FLAG_G1_COMPRESSED and bn254_batch_g1_decompress_device
// (bn254_amd/csrc/bn254_g1stage.h) — the very functions k_g1c_stage, k_g1c_overlay and k_g1c_decompress run — as a stand-alone program:
// the kernels' grids are emulated as a loop over blocks of 64 lanes with the kernels' own bound check.  Built plain, with
// -fsanitize=address,undefined and with -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb / value bound) by
// tests/test_g1_stage.py, which compares what it writes with the oracle.  Every buffer has its exact size, and the encodings start at an
// odd address, so that a sanitizer sees every access past an end and every load that assumes alignment.
//
//   hostsim_g1_stage IN OUT
//   IN : u64 n (little-endian) | n * 33 encodings | n status bytes (what a call would have written on the staged items)
//   OUT: n * 64 staged | n pre-statuses | n statuses behind the overlay | n * 64 decompressed (the _device call's bytes) | n statuses of it
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_io.h"
#include "../../bn254_amd/csrc/bn254_g1stage.h"

using namespace bn254;

static const size_t WAVE = 64;

static void k_stage(size_t block, size_t lane, const uint8_t* in33, size_t n, uint8_t* out64, uint8_t* pre) {
  const size_t i = block * WAVE + lane;
  if (i >= n) return;
  pre[i] = g1c_stage_item(out64 + 64 * i, in33 + 33 * i);
}
static void k_overlay(size_t block, size_t lane, size_t n, const uint8_t* pre, uint8_t* status) {
  const size_t i = block * WAVE + lane;
  if (i >= n) return;
  const uint8_t p = pre[i];
  if (p != ST_OK) status[i] = g1c_overlay_item(status[i], p);
}
static void k_decompress(size_t block, size_t lane, const uint8_t* in33, size_t n, uint8_t* out64, uint8_t* status) {
  const size_t i = block * WAVE + lane;
  if (i >= n) return;
  status[i] = g1c_decompress_item(out64 + 64 * i, in33 + 33 * i);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t n64 = 0;
  if (fread(&n64, 8, 1, f) != 1) { fprintf(stderr, "short input\n"); return 2; }
  const size_t n = (size_t)n64;
  // malloc'ed with their exact sizes (one byte more where n == 0 would ask for nothing); the encodings one byte into their block
  uint8_t* enc_block = (uint8_t*)malloc(33 * n + 1);
  uint8_t* enc = enc_block + 1;
  uint8_t* status = (uint8_t*)malloc(n ? n : 1);
  uint32_t* staged = (uint32_t*)malloc(n ? 64 * n : 1);
  uint32_t* plain = (uint32_t*)malloc(n ? 64 * n : 1);
  uint8_t* pre = (uint8_t*)malloc(n ? n : 1);
  uint8_t* plain_st = (uint8_t*)malloc(n ? n : 1);
  if (!enc_block || !status || !staged || !plain || !pre || !plain_st) return 2;
  if (n && (fread(enc, 33, n, f) != n || fread(status, 1, n, f) != n)) { fprintf(stderr, "short input\n"); return 2; }
  fclose(f);
  const size_t blocks = (n + WAVE - 1) / WAVE;
  for (size_t b = 0; b < blocks; ++b)
    for (size_t t = 0; t < WAVE; ++t) k_stage(b, t, enc, n, (uint8_t*)staged, pre);
  for (size_t b = 0; b < blocks; ++b)
    for (size_t t = 0; t < WAVE; ++t) k_overlay(b, t, n, pre, status);
  for (size_t b = 0; b < blocks; ++b)
    for (size_t t = 0; t < WAVE; ++t) k_decompress(b, t, enc, n, (uint8_t*)plain, plain_st);
#if defined(BN_TRACK_BOUNDS)
  if (::bn_bound_failed) { fprintf(stderr, "a limb / value bound was violated\n"); return 3; }
#endif
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  bool ok = true;
  if (n) ok = fwrite(staged, 64, n, f) == n && fwrite(pre, 1, n, f) == n && fwrite(status, 1, n, f) == n && fwrite(plain, 64, n, f) == n && fwrite(plain_st, 1, n, f) == n;
  ok = fclose(f) == 0 && ok;
  free(enc_block); free(status); free(staged); free(plain); free(pre); free(plain_st);
  if (!ok) { fprintf(stderr, "short output\n"); return 2; }
  printf("hostsim_g1_stage ok: %zu items\n", n);
  return 0;
}
