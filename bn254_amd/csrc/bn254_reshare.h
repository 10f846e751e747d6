// Linear combinations of vectors of G2 points, one scalar per vector, and the reshare of a threshold key (include/bn254_hip.h:
// bn254_batch_g2_vector_combine[_device], bn254_ctx_reshare_commitments): out[k] = sum_i scalar_i V_i[k].  The arithmetic and the
// bookkeeping of the kernels of bn254_reshare.hip, shared with their host compilation for the CPU suite (tests/hostsim: plain, under
// -DBN_TRACK_BOUNDS and as a sanitised stand-alone program).
//   * DECODE, once per point: the layout of bn254_polyeval.h (pe_decode: 4 x 9 Montgomery limbs, an identity byte, the decode status — 146 B).
//     Point k of vector i is entry i len + k.
//   * TERM (vc_term): term s = k T + r of the T len terms is scalar[pick[r]] times point k of vector pick[r] — COLUMN-major, so the terms of
//     output k are the segment [k T, (k+1) T) of the sums of bn254_batch_g2_msm (bn254_threshold.h: msm_lane_sum, msm_wave_partial,
//     msm_tree_level over G2Jac), in vector order.  T = the vectors taken: all d of them for the plain combine (pick = null: r itself), the
//     `threshold` lowest qualified dealers for the reshare.  The ladder is g2msm_ladder over the decoded limbs, as g2msm_term_key walks a
//     registered key; a lane past the end and a point that did not decode walk the generator under the identity flag.
//   * QUALIFY (rs_qualify): dealer i with key index dealer_key[i], the first that applies: the index is not below n_keys (2); the key's
//     registration status; the first non-zero decode status of its vector in coefficient order; D_i,0 is not the registered key as a GROUP
//     ELEMENT (9) — the identity flags, then fp2_eq on the coordinates, not the limb words: a decoded coordinate and a registered one are
//     both < q in value but the limbs of one value are not unique —; else 0.
//   * SELECT (rs_count, rs_prefix, rs_select_lane): one wave ranks the qualified dealers — lane l owns the dealers [l per, (l+1) per),
//     per = ceil(d / 64): every lane the count of its chunk, ONE lane the exclusive prefix of the 64 counts, every lane its chunk again — and
//     with |Q| >= t writes pick[rank] = position for rank < t and the bits of those t keys into the zeroed used row (S: the t lowest key
//     indices of Q, because dealer_key is strictly increasing); with |Q| < t the row is Q and the stop byte is raised (MSM_SEG_MASKED, the
//     `skip` convention of bn254_dealing.hip).
//   * COEFFICIENT (rs_coeff): lambda of the taken dealer's key in S by th_lagrange_row (x_j = j + 1), 32 big-endian bytes at the DEALER's
//     position, so that the term kernel reads scalar[pick[r]] in both calls.
// Scratch per term: 146 B per decoded point, the G2Jac term (216 B) and its status byte.
// Include after bn254_hash.h, bn254_io.h, bn254_pairing.h, bn254_collect.h, bn254_fr.h, bn254_threshold.h, bn254_dealing.h and bn254_polyeval.h.
#pragma once

namespace bn254 {

#define RS_ST_NOT_THE_KEY ST_VERIFICATION_FAILED

// ---- term ------------------------------------------------------------------------------------------------------------------------------------------
// term s of T len, column-major.  pick: position of the r-th taken vector (null: r).  !live (a lane past the end): the identity
BN_DEV void vc_term(G2Jac& out, uint8_t& st, const int32_t* xy, const uint8_t* inf, const uint8_t* pt_st, const uint8_t* scalars, const uint32_t* pick,
                    uint64_t T, uint64_t len, uint64_t s, bool reduce, bool live) {
  const uint64_t k = live ? s / T : 0, r = live ? s % T : 0;
  const uint64_t v = (live && pick) ? pick[r] : r;
  G2Affine p;
  pe_load(p, st, xy, inf, pt_st, v * len + k, live);
  g2msm_ladder(out, p, live && st == ST_OK, scalars + 32 * v, reduce);
}

// ---- qualify ---------------------------------------------------------------------------------------------------------------------------------------
BN_DEV bool rs_same_point(const G2Affine& a, const G2Affine& b) {
  if (a.inf || b.inf) return a.inf && b.inf;
  return fp2_eq(a.x, b.x) && fp2_eq(a.y, b.y);
}
// the status of dealer i (rules 1 to 5 of bn254_ctx_reshare_commitments)
BN_DEV uint8_t rs_qualify(const int32_t* xy, const uint8_t* inf, const uint8_t* pt_st, uint64_t len, const uint32_t* dealer_key, uint64_t i,
                          const int32_t* key_xy, const uint8_t* key_st, const uint8_t* key_inf, uint64_t n_keys) {
  const uint32_t key = dealer_key[i];
  if (key >= n_keys) return ST_INDEX_OOB;
  if (key_st[key] != ST_OK) return key_st[key];
  for (uint64_t k = 0; k < len; ++k)
    if (pt_st[i * len + k] != ST_OK) return pt_st[i * len + k];
  G2Affine d0, pk;
  uint8_t st;
  pe_load(d0, st, xy, inf, pt_st, i * len, true);
  pe_load(pk, st, key_xy, key_inf, key_st, key, true);          // a registered key lies in its table as a decoded point does in the scratch
  return rs_same_point(d0, pk) ? (uint8_t)ST_OK : (uint8_t)RS_ST_NOT_THE_KEY;
}

// ---- select ----------------------------------------------------------------------------------------------------------------------------------------
BN_DEV void rs_chunk(uint64_t d, unsigned lane, uint64_t& lo, uint64_t& hi) {
  const uint64_t per = (d + BN_CL_WAVE - 1) / BN_CL_WAVE;
  const uint64_t a = (uint64_t)lane * per, b = a + per;
  lo = a < d ? a : d;
  hi = b < d ? b : d;
}
BN_DEV uint32_t rs_count(const uint8_t* dealer_st, uint64_t d, unsigned lane) {
  uint64_t lo, hi;
  rs_chunk(d, lane, lo, hi);
  uint32_t n = 0;
  for (uint64_t i = lo; i < hi; ++i) n += dealer_st[i] == ST_OK ? 1u : 0u;
  return n;
}
// ONE lane: the 64 counts become their exclusive prefix sums, in place; returns |Q|
BN_DEV uint32_t rs_prefix(uint32_t* part) {
  uint32_t run = 0;
  for (unsigned l = 0; l < BN_CL_WAVE; ++l) { const uint32_t own = part[l]; part[l] = run; run += own; }
  return run;
}
// every lane its chunk again: rank = the qualified dealers in front.  row: bm_words zeroed words
BN_DEV void rs_select_lane(uint32_t* pick, uint32_t* row, size_t bm_words, const uint32_t* dealer_key, const uint8_t* dealer_st, uint64_t d, unsigned lane,
                           uint32_t prefix, uint32_t total, uint32_t t) {
  uint64_t lo, hi;
  rs_chunk(d, lane, lo, hi);
  uint32_t rank = prefix;
  for (uint64_t i = lo; i < hi; ++i) {
    if (dealer_st[i] != ST_OK) continue;
    const bool taken = total >= t && rank < t;
    if (taken) pick[rank] = (uint32_t)i;
    if (taken || total < t) (void)cl_claim(row, bm_words, dealer_key[i]);
    ++rank;
  }
}
// what lane 0 leaves behind the ranking: the stop byte every later kernel honours, and the call's status
BN_DEV void rs_verdict(uint8_t& skip, uint8_t& status, uint32_t total, uint32_t t) {
  skip = total >= t ? (uint8_t)0 : (uint8_t)MSM_SEG_MASKED;
  status = total >= t ? (uint8_t)ST_OK : (uint8_t)ST_VERIFICATION_FAILED;
}

// ---- coefficient -----------------------------------------------------------------------------------------------------------------------------------
// the r-th taken dealer: lambda of its key in S = the used row, at the dealer's position
BN_DEV void rs_coeff(uint8_t* scalars, const uint32_t* pick, const uint32_t* dealer_key, const uint32_t* row, size_t bm_words, uint64_t r) {
  const uint32_t i = pick[r];
  fr_to_be(scalars + 32 * (size_t)i, th_lagrange_row(row, bm_words, dealer_key[i]));
}

}  // namespace bn254
