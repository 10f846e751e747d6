// hostsim_merge — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the select-and-sum of bn254_batch_merge_keyed_bitmap (bn254_amd/csrc/bn254_merge.h) — the very functions k_mg_lane and
// k_mg_wave run.  The wave layout is emulated as the 64 lanes' select (bn254_merge.h walks the lanes' words itself where there is no wave to
// vote in), their 64 partial sums, lane after lane, plus the collect's tree.  Built plain and with -DBN_TRACK_BOUNDS (the interval tracker
// aborts on a violated limb / value bound) as a shared library by tests/test_merge_keyed_bitmap.py; and with -DHM_MAIN as a stand-alone
// program that checks itself on multiples of the generator, which is what the sanitizer build runs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_io.h"
#include "../../bn254_amd/csrc/bn254_pairing.h"
#include "../../bn254_amd/csrc/bn254_collect.h"
#include "../../bn254_amd/csrc/bn254_merge.h"

using namespace bn254;

extern "C" {

// layout 0: a lane per tuple; 1: a wave per tuple.  bits: n * bm_words zeroed words; taken: n_parts zeroed bytes.
void hm_merge(const uint8_t* parts, const uint32_t* rows, const uint64_t* off, const uint8_t* part_st, const uint8_t* tuple_st, size_t n, size_t bm_words,
              int layout, uint8_t* taken, uint32_t* bits, uint8_t* agg, uint32_t* counts) {
  const MgParts in = {parts, rows, off, part_st, tuple_st};
  for (size_t i = 0; i < n; ++i) {
    const uint64_t len = mg_tuple_len(in, i, true), lo = off[i];
    uint32_t* row = bits + i * bm_words;
    if (layout == 0) {
      G1Jac acc;
      mg_lane_walk(acc, counts[i], row, taken, bm_words, in, lo, len);
      cl_encode(agg + 64 * i, acc);
      continue;
    }
    std::vector<ClJacSlot> part(BN_CL_WAVE);
    uint32_t cnt[BN_CL_WAVE];
    mg_wave_select(row, taken, bm_words, in, lo, len, 0);
    for (unsigned t = 0; t < BN_CL_WAVE; ++t) mg_wave_partial(part[t].v, cnt[t], row, taken, bm_words, in, lo, len, t);
    for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
      for (unsigned t = 0; t < stride; ++t) cl_tree_level(part.data(), cnt, t, stride);
    cl_encode(agg + 64 * i, part[0].v);
    counts[i] = cnt[0];
  }
}

}  // extern "C"

#if defined(HM_MAIN)
// Partial p of a tuple is (p + 1) G with the bits [7 p, 7 p + 5) of a row of bm_words words (wrapped), so neighbours are disjoint and partials
// far enough apart overlap once the row is full; every fifth partial is refused.  Exact-size buffers, so that a sanitizer sees every access
// past an end.  Checks: both layouts agree byte for byte; the aggregate is (the sum of the taken p + 1) G; the count is the row's popcount.
static void multiple_of_g(uint8_t* out64, uint64_t k) {
  G1Affine g;
  g.x = fp_load_const(C_G1_GEN[0]); g.y = fp_load_const(C_G1_GEN[1]); g.inf = false;
  G1Jac acc;
  jac_set_identity(acc);
  for (uint64_t j = 0; j < k; ++j) jac_accumulate(acc, g);
  cl_encode(out64, acc);
}
int main() {
  const size_t sizes[] = {0, 1, 2, 17, 64, 65, 130}, widths[] = {0, 1, 3, 64, 65, 130};
  const size_t n = sizeof sizes / sizeof sizes[0];
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + sizes[i];
  const size_t n_parts = (size_t)off[n];
  std::vector<uint8_t> parts(64 * n_parts), part_st(n_parts), tuple_st(n, 0);
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < sizes[i]; ++k) {
      multiple_of_g(&parts[64 * (off[i] + k)], k + 1);
      part_st[off[i] + k] = k % 5 == 4 ? 9 : 0;
    }
  tuple_st[2] = 2;                                       // a refused tuple: nothing taken, the identity
  for (size_t bm_words : widths) {
    std::vector<uint32_t> rows(n_parts * bm_words, 0);
    const size_t n_bits = 32 * bm_words;
    for (size_t i = 0; i < n && n_bits; ++i)
      for (size_t k = 0; k < sizes[i]; ++k)
        for (size_t b = 0; b < 5; ++b) {
          const size_t bit = (7 * k + b) % n_bits;
          rows[(off[i] + k) * bm_words + bit / 32] |= 1u << (bit % 32);
        }
    std::vector<uint8_t> taken[2], agg[2];
    std::vector<uint32_t> bits[2], counts[2];
    for (int layout = 0; layout < 2; ++layout) {
      taken[layout].assign(n_parts, 0), agg[layout].assign(64 * n, 0xEE), bits[layout].assign(n * bm_words, 0), counts[layout].assign(n, 77);
      hm_merge(parts.data(), rows.data(), off.data(), part_st.data(), tuple_st.data(), n, bm_words, layout, taken[layout].data(), bits[layout].data(),
               agg[layout].data(), counts[layout].data());
    }
    if (taken[0] != taken[1] || agg[0] != agg[1] || bits[0] != bits[1] || counts[0] != counts[1]) { printf("layouts differ at bm_words %zu\n", bm_words); return 1; }
    for (size_t i = 0; i < n; ++i) {
      uint64_t k_sum = 0;
      uint32_t pop = 0;
      for (size_t k = 0; k < sizes[i]; ++k) k_sum += taken[0][off[i] + k] ? k + 1 : 0;
      for (size_t w = 0; w < bm_words; ++w) pop += (uint32_t)__builtin_popcount(bits[0][i * bm_words + w]);
      uint8_t want[64];
      multiple_of_g(want, k_sum);
      if (std::memcmp(want, &agg[0][64 * i], 64) != 0 || pop != counts[0][i]) { printf("tuple %zu wrong at bm_words %zu\n", i, bm_words); return 2; }
      if (tuple_st[i] == 2 && (k_sum || pop)) { printf("refused tuple %zu not empty\n", i); return 3; }
      if (bm_words == 0 && tuple_st[i] == 0 && sizes[i] && !taken[0][off[i]]) { printf("empty rows are disjoint: tuple %zu\n", i); return 4; }
    }
  }
  printf("hostsim_merge ok\n");
  return 0;
}
#endif
