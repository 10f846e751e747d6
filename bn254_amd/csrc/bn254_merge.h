// Merging partial signer-bitmap aggregates into one aggregate per message (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap[_device]):
// the select-and-sum of the call's own kernels (bn254_merge.hip), shared with their host compilation for the CPU suite (tests/hostsim,
// plain and under -DBN_TRACK_BOUNDS).  The range rule, the loads, the tree and the encoding are bn254_collect.h's.
//   * SELECT is FIRST-FIT in the caller's order: partial p of a tuple is taken iff its status is 0 and its row is disjoint from the OR of the
//     rows taken before it in that tuple (mg_overlap on the tuple's output row, then mg_or_in).  Unlike the collect's claims it is serial in
//     the partials — whether p is taken depends on every earlier decision — so only the WORDS of a row are walked in parallel.
//   * Two layouts.  A LANE walks the partials of its (short) tuple, all words of the row, one addition per taken partial, a step nobody in
//     the wave takes skipped (mg_lane_walk).  The lanes of a WAVE share one (long) tuple: lane l owns words l, l + 64, .. of the output
//     row — it alone reads and writes them, so no atomics — tests them against the partial's, one wave vote decides, and on no overlap each
//     lane ORs its words in (mg_wave_select: the test of every stride is finished before the vote, the ORs come behind it).  Then lane l
//     adds the taken partials l, l + 64, .. (mg_wave_partial, reading part_taken) and the collect's tree folds the 64 partial sums.
//   * Both layouts take the same partials and end in the same affine point, so the bytes cannot depend on the layout.
// A partial that is not taken is added as the identity under the generator's coordinates, as in the collect.  Include after bn254_collect.h.
// At the end of the file: the steps of bn254_batch_merge_keyed_bitmap_optimistic[_device] (mgo_*), which read rule 2 of bn254_bitmap.h.
#pragma once
#include "bn254_bitmap.h"

namespace bn254 {

// what the select-and-sum reads: the partials' signatures and bitmap rows, the tuples' ranges, and the two status arrays
struct MgParts { const uint8_t* parts; const uint32_t* rows; const uint64_t* off; const uint8_t* part_st; const uint8_t* tuple_st; };

// the partials of tuple i as the select-and-sum walks them: none for a tuple the range rule refused, or for a lane past the end
BN_DEV uint64_t mg_tuple_len(const MgParts& in, size_t i, bool live) {
  if (!live || in.tuple_st[i] == ST_INDEX_OOB) return 0;
  return in.off[i + 1] - in.off[i];
}

// ---- the row: words first, first + stride, .. (the lane layout: 0 and 1; the wave layout: the lane and BN_CL_WAVE) -----------------------------
BN_DEV bool mg_overlap(const uint32_t* row, const uint32_t* part, size_t bm_words, size_t first, size_t stride) {
  uint32_t hit = 0;
  for (size_t w = first; w < bm_words; w += stride) hit |= row[w] & part[w];
  return hit != 0;
}
BN_DEV void mg_or_in(uint32_t* row, const uint32_t* part, size_t bm_words, size_t first, size_t stride) {
  for (size_t w = first; w < bm_words; w += stride) row[w] |= part[w];
}
BN_DEV uint32_t mg_popcount(const uint32_t* row, size_t bm_words, size_t first, size_t stride) {
  uint32_t count = 0;
  for (size_t w = first; w < bm_words; w += stride) {
    uint32_t v = row[w];
    for (; v; v &= v - 1) ++count;
  }
  return count;
}

// ---- lane per tuple --------------------------------------------------------------------------------------------------------------------------
// one step: partial lo + k of a tuple of `len` partials, tested against and ORed into `row`; part_taken written for every partial walked
BN_DEV void mg_lane_step(G1Jac& acc, uint32_t* row, uint8_t* part_taken, size_t bm_words, const MgParts& in, uint64_t lo, uint64_t len, uint64_t k) {
  bool take = false;
  const uint64_t p = lo + k;
  if (k < len) {
    const uint32_t* part = in.rows + p * bm_words;
    take = in.part_st[p] == ST_OK && !mg_overlap(row, part, bm_words, 0, 1);
    if (take) mg_or_in(row, part, bm_words, 0, 1);
    part_taken[p] = take ? 1 : 0;
  }
  if (!BN_WAVE_ANY(take)) return;                           // a step nobody in the wave takes
  G1Affine pt;
  cl_load_share(pt, in.parts, p, take);
  jac_accumulate(acc, pt);
}
// the loop runs to the wave's longest tuple (the additions vote across the wave); a lane with len = 0 walks identities
BN_DEV void mg_lane_walk(G1Jac& acc, uint32_t& count, uint32_t* row, uint8_t* part_taken, size_t bm_words, const MgParts& in, uint64_t lo, uint64_t len) {
  jac_set_identity(acc);
  for (uint64_t k = 0; BN_WAVE_ANY(k < len); ++k) mg_lane_step(acc, row, part_taken, bm_words, in, lo, len, k);
  count = len ? mg_popcount(row, bm_words, 0, 1) : 0;
}

// ---- wave per tuple --------------------------------------------------------------------------------------------------------------------------
// select: every lane of the wave calls this with its lane number; the statuses and the votes are wave-uniform, so the lanes stay together.
// The host compilation has no wave to vote in: ONE call (lane 0) walks the 64 lanes' words itself, every lane's test before any lane's OR.
BN_DEV void mg_wave_select(uint32_t* row, uint8_t* part_taken, size_t bm_words, const MgParts& in, uint64_t lo, uint64_t len, unsigned lane) {
  for (uint64_t k = 0; k < len; ++k) {
    const uint64_t p = lo + k;
    const uint32_t* part = in.rows + p * bm_words;
    const bool ok = in.part_st[p] == ST_OK;
#if defined(__HIPCC__)
    const bool hit = ok && mg_overlap(row, part, bm_words, lane, BN_CL_WAVE);
    const bool take = ok && !BN_WAVE_ANY(hit);
    if (take) mg_or_in(row, part, bm_words, lane, BN_CL_WAVE);
#else
    bool hit = false;
    for (unsigned l = 0; ok && l < BN_CL_WAVE; ++l) hit = mg_overlap(row, part, bm_words, l, BN_CL_WAVE) || hit;
    const bool take = ok && !hit;
    for (unsigned l = 0; take && l < BN_CL_WAVE; ++l) mg_or_in(row, part, bm_words, l, BN_CL_WAVE);
#endif
    if (lane == 0) part_taken[p] = take ? 1 : 0;
  }
}
// sum: lane `lane` adds the taken partials lane, lane + 64, .. (part_taken as the select left it), and counts its own words of the finished row
BN_DEV void mg_wave_partial(G1Jac& acc, uint32_t& count, const uint32_t* row, const uint8_t* part_taken, size_t bm_words, const MgParts& in, uint64_t lo,
                            uint64_t len, unsigned lane) {
  jac_set_identity(acc);
  for (uint64_t k = lane; BN_WAVE_ANY(k < len); k += BN_CL_WAVE) {
    const bool take = k < len && part_taken[lo + k] != 0;
    if (!BN_WAVE_ANY(take)) continue;
    G1Affine pt;
    cl_load_share(pt, in.parts, lo + k, take);
    jac_accumulate(acc, pt);
  }
  count = mg_popcount(row, bm_words, lane, BN_CL_WAVE);
}

// ---- the optimistic merge (bn254_batch_merge_keyed_bitmap_optimistic[_device]) -----------------------------------------------
// The partials of a tuple share the message: if all candidates are good and pairwise disjoint, their sum is the aggregate of the union row,
// and ONE verify of the sum against the union row's keys proves it.  So: rules 1-3 per partial without a pairing or an aggregate key
// (mgo_precheck: status 0 = a CANDIDATE), the first fit above over the candidates with a refused candidate reported as an OVERLAP and the
// candidates counted (mgo_lane_step, mgo_wave_select), one flag per tuple (mgo_flag, the collect's CLO_* values), the tuple check by the
// bitmap verify's kernels, and — for the tuples that fail it or have an overlap — the exact verify of their candidates through a queue
// (clo_queued serves: it asks only for status 0 and the tuple's flag and verdict) and the exact first fit again on their zeroed rows
// (mgo_resum_len masks it: a tuple that does not go the exact way has length 0, so nothing of it is written).

// rules 1-3 of the bitmap verify for one partial of an accepted tuple, in that order: sigma's decode status (the call's flags), the lowest
// bad bit of its row, the tuple's hash status
BN_DEV uint8_t mgo_precheck(const uint8_t* part64, uint32_t flags, const uint32_t* row, size_t bm_words, const BmKeys& K, uint8_t hash_st) {
  G1Affine p;
  uint8_t st = decode_g1(p, part64, flags);
  if (st == ST_OK) st = bm_rule2_status(row, bm_words, K);
  if (st == ST_OK) st = hash_st;
  return st;
}
// the tuple's flag from what the provisional select saw.  FINAL goes by the number of candidates, not by the row: a candidate with an empty
// row leaves the row empty and still needs its check (only the identity passes it)
BN_DEV uint8_t mgo_flag(uint32_t cand, uint32_t overlap) {
  if (overlap) return CLO_EXACT;
  return cand == 0 ? CLO_FINAL : CLO_CHECK;
}
// the partials of tuple i as the masked re-select walks them: those of a tuple that goes the exact way, none of any other
BN_DEV uint64_t mgo_resum_len(const MgParts& in, size_t i, bool live, const uint8_t* flag, const uint8_t* verdict) {
  if (!live || !clo_goes_exact(flag[i], verdict[i])) return 0;
  return mg_tuple_len(in, i, true);
}
// mg_lane_step with the candidates counted and a refused candidate (ok && hit) reported
BN_DEV void mgo_lane_step(G1Jac& acc, uint32_t& cand, uint32_t& overlap, uint32_t* row, uint8_t* part_taken, size_t bm_words, const MgParts& in, uint64_t lo,
                          uint64_t len, uint64_t k) {
  bool take = false;
  const uint64_t p = lo + k;
  if (k < len) {
    const uint32_t* part = in.rows + p * bm_words;
    const bool ok = in.part_st[p] == ST_OK;
    const bool hit = ok && mg_overlap(row, part, bm_words, 0, 1);
    take = ok && !hit;
    if (take) mg_or_in(row, part, bm_words, 0, 1);
    part_taken[p] = take ? 1 : 0;
    cand += ok ? 1u : 0u;
    overlap |= hit ? 1u : 0u;
  }
  if (!BN_WAVE_ANY(take)) return;                           // a step nobody in the wave takes
  G1Affine pt;
  cl_load_share(pt, in.parts, p, take);
  jac_accumulate(acc, pt);
}
BN_DEV void mgo_lane_walk(G1Jac& acc, uint32_t& count, uint32_t& cand, uint32_t& overlap, uint32_t* row, uint8_t* part_taken, size_t bm_words, const MgParts& in,
                          uint64_t lo, uint64_t len) {
  jac_set_identity(acc);
  cand = 0;
  overlap = 0;
  for (uint64_t k = 0; BN_WAVE_ANY(k < len); ++k) mgo_lane_step(acc, cand, overlap, row, part_taken, bm_words, in, lo, len, k);
  count = len ? mg_popcount(row, bm_words, 0, 1) : 0;
}
// mg_wave_select with the same two reports; both are wave-uniform (the statuses are, and the overlap is the wave's vote).  The sum behind
// it is mg_wave_partial, unchanged.
BN_DEV void mgo_wave_select(uint32_t& cand, uint32_t& overlap, uint32_t* row, uint8_t* part_taken, size_t bm_words, const MgParts& in, uint64_t lo, uint64_t len,
                            unsigned lane) {
  cand = 0;
  overlap = 0;
  for (uint64_t k = 0; k < len; ++k) {
    const uint64_t p = lo + k;
    const uint32_t* part = in.rows + p * bm_words;
    const bool ok = in.part_st[p] == ST_OK;
#if defined(__HIPCC__)
    const bool hit = BN_WAVE_ANY(ok && mg_overlap(row, part, bm_words, lane, BN_CL_WAVE));
#else
    bool hit = false;
    for (unsigned l = 0; ok && l < BN_CL_WAVE; ++l) hit = mg_overlap(row, part, bm_words, l, BN_CL_WAVE) || hit;
#endif
    const bool take = ok && !hit;
#if defined(__HIPCC__)
    if (take) mg_or_in(row, part, bm_words, lane, BN_CL_WAVE);
#else
    for (unsigned l = 0; take && l < BN_CL_WAVE; ++l) mg_or_in(row, part, bm_words, l, BN_CL_WAVE);
#endif
    if (lane == 0) part_taken[p] = take ? 1 : 0;
    cand += ok ? 1u : 0u;
    overlap |= hit ? 1u : 0u;
  }
}

}  // namespace bn254
