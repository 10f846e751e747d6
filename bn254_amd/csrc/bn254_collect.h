// Building signer-bitmap aggregates from the signers' individual signatures (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap[_device],
// and at the end of the file the steps of bn254_batch_collect_keyed_bitmap_optimistic[_device]):
// the bookkeeping and the arithmetic of the call's own kernels (bn254_collect.hip), shared with their host compilation for the CPU suite
// (tests/hostsim, plain and under -DBN_TRACK_BOUNDS).  Written against the jac_* interface of bn254_curve.h and the
// decoders of bn254_io.h; G1 only, so it is the same in both layouts of Fq2.
//   * the RANGE RULE of the _device form (that of bn254_batch_aggregate_verify_distinct_device): tuple i's shares [off[i], off[i+1]) are
//     accepted iff off[i] <= off[i+1] <= n_shares and no earlier offset exceeds off[i].  Accepted ranges are disjoint and ascending, so the
//     prefix maximum `end` of the accepted ranges' ends is monotone and a share finds its tuple by a binary search of it (cl_tuple_of).
//   * SELECT: share s counts iff its status is 0 and no earlier counted share of its tuple named the same key — the test-and-set of bit
//     share_key[s] in the tuple's output row (cl_claim).  Which of several valid shares of one key is taken does not matter: G1 has prime
//     order, so the valid signature of (m, pk) is unique and the duplicates are the same point.  That is what lets the lanes of a wave
//     claim in any order.
//   * SUM, two layouts: a LANE walks the shares of its (short) tuple in order, one addition per counted share, a step none of the wave's
//     lanes counts skipped (cl_lane_sum); the lanes of a WAVE take the shares l, l + 64, .. of one (long) tuple, each its own partial sum
//     (cl_wave_partial), and a tree of six levels of full Jacobian additions folds the 64 partial sums (cl_tree_level).  Both layouts end in
//     the same affine point, so the bytes cannot depend on the layout or on the order of the claims.
// A share that does not count is added as the identity under the generator's coordinates (never (0, 0)), so the wave stays convergent.
// Include after bn254_io.h.
#pragma once

namespace bn254 {

// what the select-and-sum reads — only what the caller sees: the shares, their key indices, the tuples' ranges, and the two status arrays
struct ClShares { const uint8_t* shares; const uint32_t* key; const uint64_t* off; const uint8_t* share_st; const uint8_t* tuple_st; };

// ---- the range rule ------------------------------------------------------------------------------------------------------------------------
// mx_before = the maximum of off[0 .. i - 1] (unused for i = 0)
BN_DEV bool cl_range_ok(uint64_t lo, uint64_t hi, uint64_t n_shares, bool first, uint64_t mx_before) {
  return lo <= hi && hi <= n_shares && (first || mx_before <= lo);
}
// share s -> its tuple, or n when it belongs to no accepted tuple.  end[i] = the largest end of an accepted range among tuples 0 .. i (0:
// none): the first i with end[i] > s is accepted and ends behind s; it holds s iff it starts at or before s.
BN_DEV size_t cl_tuple_of(uint64_t s, const uint64_t* end, const uint64_t* off, size_t n) {
  size_t a = 0, b = n;
  while (a < b) {
    const size_t mid = (a + b) >> 1;
    if (end[mid] > s) b = mid; else a = mid + 1;
  }
  return a < n && off[a] <= s ? a : n;
}
// the shares of tuple i as the select-and-sum walks them: none for a tuple the range rule refused (status 2), or for a lane past the end
BN_DEV uint64_t cl_tuple_len(const ClShares& in, size_t i, bool live) {
  if (!live || in.tuple_st[i] == ST_INDEX_OOB) return 0;
  return in.off[i + 1] - in.off[i];
}

// ---- select ----------------------------------------------------------------------------------------------------------------------------------
// test-and-set of bit `key` of a zeroed row of bm_words words: true iff this call set it.  The lanes of a wave share the row in the wave
// layout, hence the (vector) atomic; the host compilation runs one lane at a time.
BN_DEV bool cl_claim(uint32_t* row, size_t bm_words, uint32_t key) {
  if ((size_t)(key >> 5) >= bm_words) return false;          // not reachable behind status 0 (key < n_keys <= 32 bm_words); the row's bound all the same
  const uint32_t bit = 1u << (key & 31u);
#if defined(__HIPCC__)
  return (atomicOr(&row[key >> 5], bit) & bit) == 0;
#else
  const uint32_t old = row[key >> 5];
  row[key >> 5] = old | bit;
  return (old & bit) == 0;
#endif
}
// share s as a summand: the point when `take`, else the identity (under the generator's coordinates)
BN_DEV void cl_load_share(G1Affine& p, const uint8_t* shares, uint64_t s, bool take) {
  if (take) { (void)decode_g1(p, shares + 64 * s, 0); return; }      // status 0 behind the verify: it decodes, and to a point of the curve
  p.x = fp_load_const(C_G1_GEN[0]); p.y = fp_load_const(C_G1_GEN[1]); p.inf = true;
}
// one step of either walk: share lo + k of a tuple of `len` shares, claimed in `row`
BN_DEV void cl_step(G1Jac& acc, uint32_t& count, uint32_t* row, size_t bm_words, const ClShares& in, uint64_t lo, uint64_t len, uint64_t k) {
  bool take = false;
  const uint64_t s = lo + k;
  if (k < len && in.share_st[s] == ST_OK) take = cl_claim(row, bm_words, in.key[s]);
  if (!BN_WAVE_ANY(take)) return;                           // a step nobody in the wave counts
  G1Affine p;
  cl_load_share(p, in.shares, s, take);
  jac_accumulate(acc, p);
  count += take ? 1u : 0u;
}

// ---- sum -------------------------------------------------------------------------------------------------------------------------------------
// lane per tuple: the loop runs to the wave's longest tuple (the additions vote across the wave); a lane with len = 0 walks identities
BN_DEV void cl_lane_sum(G1Jac& acc, uint32_t& count, uint32_t* row, size_t bm_words, const ClShares& in, uint64_t lo, uint64_t len) {
  jac_set_identity(acc);
  count = 0;
  for (uint64_t k = 0; BN_WAVE_ANY(k < len); ++k) cl_step(acc, count, row, bm_words, in, lo, len, k);
}
// wave per tuple: lane `lane` of BN_CL_WAVE takes the shares lane, lane + 64, ..
#define BN_CL_WAVE 64
BN_DEV void cl_wave_partial(G1Jac& acc, uint32_t& count, uint32_t* row, size_t bm_words, const ClShares& in, uint64_t lo, uint64_t len, unsigned lane) {
  jac_set_identity(acc);
  count = 0;
  for (uint64_t k = lane; BN_WAVE_ANY(k < len); k += BN_CL_WAVE) cl_step(acc, count, row, bm_words, in, lo, len, k);
}
// one level of the tree over the partial sums (slots with a member v, counts beside them): slot t takes in slot t + stride
template <class Slot>
BN_DEV void cl_tree_level(Slot* part, uint32_t* cnt, unsigned t, unsigned stride) {
  jac_add(part[t].v, part[t].v, part[t + stride].v);
  cnt[t] += cnt[t + stride];
}
// the slot of a partial sum in LDS, padded like G1JacSlot of the randomised verify (bn254_rand.hip); and the block cap of the wave-per-tuple
// kernels, which reach the tuples beyond the grid by stride (k_cl_sum_wave, k_clo_sum_wave; bn254_merge.hip: k_mg_wave)
struct ClJacSlot { G1Jac v; int32_t pad; };
#define CL_WAVE_MAX_BLOCKS ((size_t)65536)
// the aggregate as the caller gets it: uncompressed, the identity as 64 zero bytes
BN_DEV void cl_encode(uint8_t* out64, const G1Jac& acc) {
  G1Affine r;
  jac_to_affine(r, acc);
  encode_g1(out64, r);
}

// ---- the optimistic collect (bn254_batch_collect_keyed_bitmap_optimistic[_device]) ---------------------------------------------------------
// The shares of a tuple share the message: if all of them are good, their sum is the aggregate of the tuple's bitmap, and ONE verify of the
// sum against the sum of the keys proves it.  So: rules 1-3 per share without a pairing (clo_precheck: status 0 = a CANDIDATE), a
// provisional select-and-sum of the candidates that reports a refused claim as a DUPLICATE (clo_step), one flag per tuple (clo_flag), the
// tuple check by the bitmap verify's kernels, and — for the tuples that fail it, have a duplicate or too few candidates — the exact keyed
// verify of their candidates through a queue (clo_queued) and the exact select-and-sum again on their zeroed rows (clo_goes_exact masks
// it; the rows and aggregates of passing tuples are not touched).
#define CLO_FINAL 0   // no candidate: empty row, identity, 0 — final as it stands
#define CLO_CHECK 1   // eligible: the provisional outputs stand iff the tuple check says 0
#define CLO_EXACT 2   // a duplicate, or fewer candidates than the per-tuple minimum: the exact way, whatever the check says

// rules 1-3 of the exact collect for one share of an accepted tuple: decode (the call's flags), key index and registration status, the
// tuple's hash status
BN_DEV uint8_t clo_precheck(const uint8_t* share64, uint32_t flags, uint32_t key, const uint8_t* key_st, uint32_t n_keys, uint8_t hash_st) {
  G1Affine p;
  uint8_t st = decode_g1(p, share64, flags);
  if (st == ST_OK) st = key >= n_keys ? (uint8_t)ST_INDEX_OOB : key_st[key];
  if (st == ST_OK) st = hash_st;
  return st;
}
// cl_step with the refused claim reported: a candidate whose bit another candidate of the tuple holds already.  (The tuple then goes the
// exact way, so which of the two was taken never shows.)
BN_DEV void clo_step(G1Jac& acc, uint32_t& count, uint32_t& dup, uint32_t* row, size_t bm_words, const ClShares& in, uint64_t lo, uint64_t len, uint64_t k) {
  bool take = false;
  const uint64_t s = lo + k;
  if (k < len && in.share_st[s] == ST_OK) {
    take = cl_claim(row, bm_words, in.key[s]);
    if (!take) dup = 1u;
  }
  if (!BN_WAVE_ANY(take)) return;
  G1Affine p;
  cl_load_share(p, in.shares, s, take);
  jac_accumulate(acc, p);
  count += take ? 1u : 0u;
}
BN_DEV void clo_lane_sum(G1Jac& acc, uint32_t& count, uint32_t& dup, uint32_t* row, size_t bm_words, const ClShares& in, uint64_t lo, uint64_t len) {
  jac_set_identity(acc);
  count = 0;
  dup = 0;
  for (uint64_t k = 0; BN_WAVE_ANY(k < len); ++k) clo_step(acc, count, dup, row, bm_words, in, lo, len, k);
}
BN_DEV void clo_wave_partial(G1Jac& acc, uint32_t& count, uint32_t& dup, uint32_t* row, size_t bm_words, const ClShares& in, uint64_t lo, uint64_t len,
                             unsigned lane) {
  jac_set_identity(acc);
  count = 0;
  dup = 0;
  for (uint64_t k = lane; BN_WAVE_ANY(k < len); k += BN_CL_WAVE) clo_step(acc, count, dup, row, bm_words, in, lo, len, k);
}
template <class Slot>
BN_DEV void clo_tree_level(Slot* part, uint32_t* cnt, uint32_t* dup, unsigned t, unsigned stride) {
  cl_tree_level(part, cnt, t, stride);
  dup[t] |= dup[t + stride];
}
// the tuple's flag from what the provisional sum saw: `count` claims (= candidates, when none was refused), min_tuple = the per-tuple minimum
BN_DEV uint8_t clo_flag(uint32_t count, uint32_t dup, uint32_t min_tuple) {
  if (dup) return CLO_EXACT;
  if (count == 0) return CLO_FINAL;
  return count < min_tuple ? CLO_EXACT : CLO_CHECK;
}
// does tuple i go the exact way, given its flag and the tuple check's verdict (read for CLO_CHECK only)
BN_DEV bool clo_goes_exact(uint8_t flag, uint8_t verdict) { return flag == CLO_EXACT || (flag == CLO_CHECK && verdict != ST_OK); }
// is share s — status share_st behind the pre-check, of tuple t (n = of nobody) — queued for the exact verify
BN_DEV bool clo_queued(uint8_t share_st, size_t t, size_t n, const uint8_t* flag, const uint8_t* verdict) {
  return t < n && share_st == ST_OK && clo_goes_exact(flag[t], verdict[t]);
}
// the shares of tuple i as the masked re-sum walks them: those of a tuple that goes the exact way, none of any other
BN_DEV uint64_t clo_resum_len(const ClShares& in, size_t i, bool live, const uint8_t* flag, const uint8_t* verdict) {
  if (!live || !clo_goes_exact(flag[i], verdict[i])) return 0;
  return cl_tuple_len(in, i, true);
}

}  // namespace bn254
