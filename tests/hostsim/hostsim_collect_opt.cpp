// hostsim_collect_opt — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the device functions of bn254_batch_collect_keyed_bitmap_optimistic (bn254_amd/csrc/bn254_collect.h: clo_*) — the
// very functions k_clo_precheck, k_clo_sum_lane, k_clo_sum_wave, k_clo_settle and k_clo_queue run — over GIVEN arrays.  The wave layout is
// emulated as its 64 partial sums, lane after lane, plus the tree.  Built plain and with -DBN_TRACK_BOUNDS by
// tests/test_collect_keyed_bitmap_optimistic.py.
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

// the prefix maximum of the accepted ranges' ends, as k_cl_plan and the scan leave it (tuple_st[i] == 2: refused)
static std::vector<uint64_t> ends_of(const uint64_t* off, const uint8_t* tuple_st, size_t n) {
  std::vector<uint64_t> end(n + 1, 0);
  uint64_t e = 0;
  for (size_t i = 0; i < n; ++i) {
    if (tuple_st[i] != ST_INDEX_OOB && off[i + 1] > e) e = off[i + 1];
    end[i] = e;
  }
  return end;
}

extern "C" {

// k_clo_precheck: share_st comes in filled with 2; hash_st per tuple
void hco_precheck(const uint8_t* shares, const uint32_t* keys, const uint64_t* off, const uint8_t* tuple_st, const uint8_t* hash_st, size_t n,
                  uint64_t n_shares, uint32_t flags, const uint8_t* key_st, uint32_t n_keys, uint8_t* share_st) {
  const std::vector<uint64_t> end = ends_of(off, tuple_st, n);
  for (uint64_t s = 0; s < n_shares; ++s) {
    const size_t t = cl_tuple_of(s, end.data(), off, n);
    if (t >= n) continue;
    share_st[s] = clo_precheck(shares + 64 * s, flags, keys[s], key_st, n_keys, hash_st[t]);
  }
}
// k_clo_sum_lane (layout 0) / k_clo_sum_wave (layout 1) over every tuple.  verdict == nullptr: the provisional sum (bits zeroed; writes
// flag); else the re-sum of the tuples that go the exact way (their rows zeroed by hco_settle), which leaves every other tuple's outputs alone
void hco_sum(const uint8_t* shares, const uint32_t* keys, const uint64_t* off, const uint8_t* share_st, const uint8_t* tuple_st, size_t n,
             size_t bm_words, int layout, uint32_t min_tuple, const uint8_t* verdict, uint8_t* flag, uint32_t* bits, uint8_t* agg, uint32_t* counts) {
  const ClShares in = {shares, keys, off, share_st, tuple_st};
  for (size_t i = 0; i < n; ++i) {
    const uint64_t len = verdict ? clo_resum_len(in, i, true, flag, verdict) : cl_tuple_len(in, i, true), lo = off[i];
    if (verdict && !clo_goes_exact(flag[i], verdict[i])) continue;
    uint32_t* row = bits + i * bm_words;
    uint32_t count, dup;
    if (layout == 0) {
      G1Jac acc;
      clo_lane_sum(acc, count, dup, row, bm_words, in, lo, len);
      cl_encode(agg + 64 * i, acc);
    } else {
      std::vector<Slot> part(BN_CL_WAVE);
      uint32_t cnt[BN_CL_WAVE], dupf[BN_CL_WAVE];
      for (unsigned t = 0; t < BN_CL_WAVE; ++t) clo_wave_partial(part[t].v, cnt[t], dupf[t], row, bm_words, in, lo, len, t);
      for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
        for (unsigned t = 0; t < stride; ++t) clo_tree_level(part.data(), cnt, dupf, t, stride);
      cl_encode(agg + 64 * i, part[0].v);
      count = cnt[0];
      dup = dupf[0];
    }
    counts[i] = count;
    if (!verdict) flag[i] = clo_flag(count, dup, min_tuple);
  }
}
// k_clo_settle: the rows of the tuples that go the exact way zeroed; stats = {checked, passed, sent the exact way}
void hco_settle(size_t n, size_t bm_words, const uint8_t* flag, const uint8_t* verdict, uint32_t* bits, uint32_t* stats) {
  stats[0] = stats[1] = stats[2] = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool checked = flag[i] == CLO_CHECK, exact = clo_goes_exact(flag[i], verdict[i]);
    if (exact) for (size_t w = 0; w < bm_words; ++w) bits[i * bm_words + w] = 0;
    stats[0] += checked, stats[1] += checked && verdict[i] == ST_OK, stats[2] += exact;
  }
}
// k_clo_queue over the slice [base, base + len): the queued slots (slice-relative), in ascending order -> their number
uint64_t hco_queue(const uint64_t* off, const uint8_t* tuple_st, size_t n, uint64_t base, uint64_t len, const uint8_t* share_st, const uint8_t* flag,
                   const uint8_t* verdict, uint32_t* list) {
  const std::vector<uint64_t> end = ends_of(off, tuple_st, n);
  uint64_t cnt = 0;
  for (uint64_t j = 0; j < len; ++j)
    if (clo_queued(share_st[base + j], cl_tuple_of(base + j, end.data(), off, n), n, flag, verdict)) list[cnt++] = (uint32_t)j;
  return cnt;
}

}  // extern "C"
