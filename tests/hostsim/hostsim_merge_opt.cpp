// hostsim_merge_opt — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the device functions of bn254_batch_merge_keyed_bitmap_optimistic (bn254_amd/csrc/bn254_merge.h: mgo_*, with
// bn254_collect.h's clo_goes_exact / clo_queued and bn254_bitmap.h's rule 2) — the very functions k_mgo_precheck, k_mgo_lane, k_mgo_wave and,
// shared with the optimistic collect, k_clo_settle and k_clo_queue run — over GIVEN arrays.  The wave layout is emulated as the 64 lanes' select, their partial sums, lane after
// lane, plus the collect's tree.  Built plain and with -DBN_TRACK_BOUNDS as a shared library by tests/test_merge_keyed_bitmap_optimistic.py;
// and with -DHMO_MAIN as a stand-alone program that checks itself on multiples of the generator, which is what the sanitizer build runs.
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

// k_mgo_precheck: part_st comes in filled with 2; hash_st per tuple; the bad-bit vector as k_bm_bad_words builds it
void hmo_precheck(const uint8_t* parts, const uint32_t* rows, const uint64_t* off, const uint8_t* tuple_st, const uint8_t* hash_st, size_t n, uint64_t n_parts,
                  size_t bm_words, uint32_t flags, const uint8_t* key_st, uint32_t n_keys, uint8_t* part_st) {
  const std::vector<uint64_t> end = ends_of(off, tuple_st, n);
  std::vector<uint32_t> bad((n_keys + 31) / 32 + 1, 0);
  for (uint32_t w = 0; w < (n_keys + 31) / 32; ++w) bad[w] = bm_bad_word(key_st, n_keys, w);
  const BmKeys K = {nullptr, key_st, nullptr, bad.data(), n_keys};
  for (uint64_t p = 0; p < n_parts; ++p) {
    const size_t t = cl_tuple_of(p, end.data(), off, n);
    if (t >= n) continue;
    part_st[p] = mgo_precheck(parts + 64 * p, flags, rows + p * bm_words, bm_words, K, hash_st[t]);
  }
}
// k_mgo_lane (layout 0) / k_mgo_wave (layout 1) over every tuple.  verdict == nullptr: the provisional select-and-sum (bits and taken zeroed;
// writes flag); else the re-select of the tuples that go the exact way (their rows zeroed by hmo_settle), which leaves every other tuple's
// outputs alone
void hmo_select(const uint8_t* parts, const uint32_t* rows, const uint64_t* off, const uint8_t* part_st, const uint8_t* tuple_st, size_t n, size_t bm_words,
                int layout, const uint8_t* verdict, uint8_t* flag, uint8_t* taken, uint32_t* bits, uint8_t* agg, uint32_t* counts) {
  const MgParts in = {parts, rows, off, part_st, tuple_st};
  for (size_t i = 0; i < n; ++i) {
    const uint64_t len = verdict ? mgo_resum_len(in, i, true, flag, verdict) : mg_tuple_len(in, i, true), lo = off[i];
    if (verdict && !clo_goes_exact(flag[i], verdict[i])) continue;
    uint32_t* row = bits + i * bm_words;
    uint32_t count, cand, overlap;
    if (layout == 0) {
      G1Jac acc;
      mgo_lane_walk(acc, count, cand, overlap, row, taken, bm_words, in, lo, len);
      cl_encode(agg + 64 * i, acc);
    } else {
      std::vector<ClJacSlot> part(BN_CL_WAVE);
      uint32_t cnt[BN_CL_WAVE];
      mgo_wave_select(cand, overlap, row, taken, bm_words, in, lo, len, 0);
      for (unsigned t = 0; t < BN_CL_WAVE; ++t) mg_wave_partial(part[t].v, cnt[t], row, taken, bm_words, in, lo, len, t);
      for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
        for (unsigned t = 0; t < stride; ++t) cl_tree_level(part.data(), cnt, t, stride);
      cl_encode(agg + 64 * i, part[0].v);
      count = cnt[0];
    }
    counts[i] = count;
    if (!verdict) flag[i] = mgo_flag(cand, overlap);
  }
}
// k_clo_settle: the rows of the tuples that go the exact way zeroed; stats = {checked, passed, sent the exact way}
void hmo_settle(size_t n, size_t bm_words, const uint8_t* flag, const uint8_t* verdict, uint32_t* bits, uint32_t* stats) {
  stats[0] = stats[1] = stats[2] = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool checked = flag[i] == CLO_CHECK, exact = clo_goes_exact(flag[i], verdict[i]);
    if (exact) for (size_t w = 0; w < bm_words; ++w) bits[i * bm_words + w] = 0;
    stats[0] += checked, stats[1] += checked && verdict[i] == ST_OK, stats[2] += exact;
  }
}
// k_clo_queue over the slice [base, base + len): the queued slots (slice-relative), in ascending order -> their number
uint64_t hmo_queue(const uint64_t* off, const uint8_t* tuple_st, size_t n, uint64_t base, uint64_t len, const uint8_t* part_st, const uint8_t* flag,
                   const uint8_t* verdict, uint32_t* list) {
  const std::vector<uint64_t> end = ends_of(off, tuple_st, n);
  uint64_t cnt = 0;
  for (uint64_t j = 0; j < len; ++j)
    if (clo_queued(part_st[base + j], cl_tuple_of(base + j, end.data(), off, n), n, flag, verdict)) list[cnt++] = (uint32_t)j;
  return cnt;
}

}  // extern "C"

#if defined(HMO_MAIN)
// Partial k of a tuple is (k + 1) G with the bits [7 k, 7 k + 5) of a row of bm_words words (wrapped), so neighbours are disjoint and partials
// far enough apart overlap once the row is full; every fifth partial is no candidate (a bit beyond the key set: the pre-check itself gives
// the 2).  Exact-size buffers, so that a sanitizer sees every access past an end.  Checks: the pre-check's statuses; both layouts agree byte
// for byte, flags included; a tuple is EXACT iff a candidate was not taken, FINAL iff it has none; the aggregate is (the sum of the taken
// k + 1) G; the queue of a given verdict holds exactly the candidates of the tuples that go the exact way; the re-select over those tuples
// reproduces the provisional outputs (the statuses did not change) and leaves a marker in every other tuple's outputs alone.
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
  std::vector<uint8_t> parts(64 * n_parts), tuple_st(n, 0);
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < sizes[i]; ++k) multiple_of_g(&parts[64 * (off[i] + k)], k + 1);
  tuple_st[2] = 2;                                       // a refused tuple: its partials keep the 2 of the fill, nothing taken, the identity
  for (size_t bm_words : widths) {
    const size_t n_bits = 32 * bm_words;
    const uint32_t n_keys = n_bits ? (uint32_t)(n_bits - 1) : 0;   // the row's last bit is beyond the set
    std::vector<uint8_t> key_st(n_keys + 1, 0);
    std::vector<uint32_t> rows(n_parts * bm_words, 0);
    for (size_t i = 0; i < n && n_bits; ++i)
      for (size_t k = 0; k < sizes[i]; ++k) {
        for (size_t b = 0; b < 5; ++b) {
          const size_t bit = (7 * k + b) % (n_bits - 1);
          rows[(off[i] + k) * bm_words + bit / 32] |= 1u << (bit % 32);
        }
        if (k % 5 == 4) rows[(off[i] + k) * bm_words + (n_bits - 1) / 32] |= 1u << ((n_bits - 1) % 32);
      }
    std::vector<uint8_t> part_st(n_parts, 2);
    hmo_precheck(parts.data(), rows.data(), off.data(), tuple_st.data(), tuple_st.data(), n, n_parts, bm_words, 0, key_st.data(), n_keys, part_st.data());
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < sizes[i]; ++k)
        if (part_st[off[i] + k] != (tuple_st[i] == 2 || (n_bits && k % 5 == 4) ? 2 : 0)) { printf("pre-check wrong at bm_words %zu\n", bm_words); return 5; }
    std::vector<uint8_t> taken[2], agg[2], flag[2];
    std::vector<uint32_t> bits[2], counts[2];
    for (int layout = 0; layout < 2; ++layout) {
      taken[layout].assign(n_parts, 0), agg[layout].assign(64 * n, 0xEE), bits[layout].assign(n * bm_words, 0), counts[layout].assign(n, 77);
      flag[layout].assign(n, 0xEE);
      hmo_select(parts.data(), rows.data(), off.data(), part_st.data(), tuple_st.data(), n, bm_words, layout, nullptr, flag[layout].data(), taken[layout].data(),
                 bits[layout].data(), agg[layout].data(), counts[layout].data());
    }
    if (taken[0] != taken[1] || agg[0] != agg[1] || bits[0] != bits[1] || counts[0] != counts[1] || flag[0] != flag[1]) {
      printf("layouts differ at bm_words %zu\n", bm_words);
      return 1;
    }
    for (size_t i = 0; i < n; ++i) {
      uint64_t k_sum = 0;
      uint32_t pop = 0, cand = 0, refused = 0;
      for (size_t k = 0; k < sizes[i]; ++k) {
        k_sum += taken[0][off[i] + k] ? k + 1 : 0;
        cand += part_st[off[i] + k] == 0, refused += part_st[off[i] + k] == 0 && !taken[0][off[i] + k];
      }
      for (size_t w = 0; w < bm_words; ++w) pop += (uint32_t)__builtin_popcount(bits[0][i * bm_words + w]);
      uint8_t want[64];
      multiple_of_g(want, k_sum);
      if (std::memcmp(want, &agg[0][64 * i], 64) != 0 || pop != counts[0][i]) { printf("tuple %zu wrong at bm_words %zu\n", i, bm_words); return 2; }
      if (flag[0][i] != (refused ? CLO_EXACT : cand ? CLO_CHECK : CLO_FINAL)) { printf("flag of tuple %zu wrong at bm_words %zu\n", i, bm_words); return 3; }
      if (bm_words == 0 && tuple_st[i] == 0 && sizes[i] && flag[0][i] != CLO_CHECK) { printf("empty rows are candidates: tuple %zu\n", i); return 4; }
    }
    // a verdict: every other CHECK tuple fails; the queue, whole and in slices of 37; the re-select
    std::vector<uint8_t> verdict(n, 0xEE);
    for (size_t i = 0; i < n; ++i) verdict[i] = i % 2 ? 9 : 0;
    std::vector<uint32_t> settled = bits[0], stats(3), list(n_parts), sliced(n_parts);
    hmo_settle(n, bm_words, flag[0].data(), verdict.data(), settled.data(), stats.data());
    const uint64_t q = hmo_queue(off.data(), tuple_st.data(), n, 0, n_parts, part_st.data(), flag[0].data(), verdict.data(), list.data());
    uint64_t q2 = 0, want_q = 0;
    for (size_t lo = 0; lo < n_parts; lo += 37) {
      std::vector<uint32_t> piece(37);
      const uint64_t len = n_parts - lo < 37 ? n_parts - lo : 37;
      const uint64_t got = hmo_queue(off.data(), tuple_st.data(), n, lo, len, part_st.data(), flag[0].data(), verdict.data(), piece.data());
      for (uint64_t j = 0; j < got; ++j) sliced[q2++] = (uint32_t)(lo + piece[j]);
    }
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < sizes[i]; ++k)
        if (clo_goes_exact(flag[0][i], verdict[i]) && part_st[off[i] + k] == 0) {
          if (want_q >= q || list[want_q] != off[i] + k) { printf("queue wrong at bm_words %zu\n", bm_words); return 6; }
          ++want_q;
        }
    if (want_q != q || q2 != q || !std::equal(list.begin(), list.begin() + q, sliced.begin())) { printf("queue length wrong at bm_words %zu\n", bm_words); return 7; }
    for (int layout = 0; layout < 2; ++layout) {
      std::vector<uint8_t> t2 = taken[0], a2 = agg[0], f2 = flag[0];
      std::vector<uint32_t> b2 = settled, c2 = counts[0];
      for (size_t i = 0; i < n; ++i) {
        if (clo_goes_exact(flag[0][i], verdict[i])) {
          for (size_t k = 0; k < sizes[i]; ++k) t2[off[i] + k] = 0x55;      // the re-select rewrites part_taken for all of these
          std::memset(&a2[64 * i], 0x77, 64);
        } else {
          std::memset(&a2[64 * i], 0xA5, 64);                                // ... and leaves a passing tuple's marker alone
          for (size_t k = 0; k < sizes[i]; ++k) t2[off[i] + k] = 0xA5;
          c2[i] = 0xA5A5;
          if (bm_words) b2[i * bm_words] ^= 0x80000000u;
        }
      }
      const std::vector<uint8_t> t_mark = t2, a_mark = a2;
      const std::vector<uint32_t> b_mark = b2, c_mark = c2;
      hmo_select(parts.data(), rows.data(), off.data(), part_st.data(), tuple_st.data(), n, bm_words, layout, verdict.data(), f2.data(), t2.data(), b2.data(),
                 a2.data(), c2.data());
      if (f2 != flag[0]) { printf("the re-select wrote a flag at bm_words %zu\n", bm_words); return 8; }
      for (size_t i = 0; i < n; ++i) {
        const bool exact = clo_goes_exact(flag[0][i], verdict[i]);
        const bool same_agg = std::memcmp(&a2[64 * i], exact ? &agg[0][64 * i] : &a_mark[64 * i], 64) == 0;
        bool same = same_agg && c2[i] == (exact ? counts[0][i] : c_mark[i]);
        for (size_t w = 0; w < bm_words; ++w) same = same && b2[i * bm_words + w] == (exact ? bits[0][i * bm_words + w] : b_mark[i * bm_words + w]);
        for (size_t k = 0; k < sizes[i]; ++k) same = same && t2[off[i] + k] == (exact ? taken[0][off[i] + k] : t_mark[off[i] + k]);
        if (!same) { printf("re-select wrong at tuple %zu, bm_words %zu, layout %d\n", i, bm_words, layout); return 9; }
      }
    }
  }
  printf("hostsim_merge_opt ok\n");
  return 0;
}
#endif
