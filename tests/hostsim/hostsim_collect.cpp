// hostsim_collect — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the select-and-sum and of the range rule of bn254_batch_collect_keyed_bitmap (bn254_amd/csrc/bn254_collect.h) — the
// very functions k_cl_sum_lane, k_cl_sum_wave, k_cl_plan and k_cl_spread run.  The wave layout is emulated as its 64 partial sums, lane
// after lane, plus the tree.  Built plain and with -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb / value bound) by
// tests/test_collect_keyed_bitmap.py.
#include <cstdint>
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

using namespace bn254;

struct Slot { G1Jac v; int32_t pad; };

extern "C" {

// layout 0: a lane per tuple; 1: a wave per tuple (64 partial sums and the tree).  bits: n * bm_words zeroed words.
void hc_sum(const uint8_t* shares, const uint32_t* keys, const uint64_t* off, const uint8_t* share_st, const uint8_t* tuple_st, size_t n,
            size_t bm_words, int layout, uint32_t* bits, uint8_t* agg, uint32_t* counts) {
  const ClShares in = {shares, keys, off, share_st, tuple_st};
  for (size_t i = 0; i < n; ++i) {
    const uint64_t len = cl_tuple_len(in, i, true), lo = off[i];
    uint32_t* row = bits + i * bm_words;
    if (layout == 0) {
      G1Jac acc;
      cl_lane_sum(acc, counts[i], row, bm_words, in, lo, len);
      cl_encode(agg + 64 * i, acc);
      continue;
    }
    std::vector<Slot> part(BN_CL_WAVE);
    uint32_t cnt[BN_CL_WAVE];
    for (unsigned t = 0; t < BN_CL_WAVE; ++t) cl_wave_partial(part[t].v, cnt[t], row, bm_words, in, lo, len, t);
    for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
      for (unsigned t = 0; t < stride; ++t) cl_tree_level(part.data(), cnt, t, stride);
    cl_encode(agg + 64 * i, part[0].v);
    counts[i] = cnt[0];
  }
}
// the range rule and the share -> tuple map as k_cl_plan and k_cl_spread compute them: ok[i], and tuple_of[s] (n for a share of nobody)
void hc_plan(const uint64_t* off, size_t n, uint64_t n_shares, uint8_t* ok, uint64_t* tuple_of) {
  std::vector<uint64_t> end(n + 1, 0);
  uint64_t mx = 0, e = 0;
  for (size_t i = 0; i < n; ++i) {
    ok[i] = cl_range_ok(off[i], off[i + 1], n_shares, i == 0, mx);
    mx = off[i] > mx ? off[i] : mx;
    if (ok[i] && off[i + 1] > e) e = off[i + 1];
    end[i] = e;
  }
  for (uint64_t s = 0; s < n_shares; ++s) tuple_of[s] = cl_tuple_of(s, end.data(), off, n);
}

}  // extern "C"
