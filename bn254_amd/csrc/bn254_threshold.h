// Threshold signatures and the segmented scalar-weighted sum in G1 (include/bn254_hip.h: bn254_batch_threshold_combine_keyed[_device],
// bn254_batch_g1_msm[_device]): the bookkeeping and the arithmetic of the kernels of bn254_threshold.hip, shared with their host compilation
// for the CPU suite (tests/hostsim, plain, under -DBN_TRACK_BOUNDS and as a sanitised stand-alone program).
//   * RANK AND SELECT: the collect's claim pass leaves row V of a tuple (bit j = key j has a status-0 share).  |V| >= t: the row is cut
//     down to its t LOWEST bits (th_trim) — a choice that depends on nothing but V, so the bytes are reproducible — and a share is KEPT iff
//     its status is 0 and its key's bit survived (th_bit): a key survives iff fewer than t bits of the row lie below it, counted across
//     word boundaries.  Of several kept shares of one key exactly one claims the key's bit in a second, zeroed row (cl_claim): they are the
//     same point (bn254_collect.h), so it does not matter which.
//   * COEFFICIENT: key j stands for the evaluation point x_j = j + 1, so key 0 is a legal signer.  lambda_j(S) = prod x_k / prod (x_k - x_j)
//     over the k != j of S, mod r: 2 (t - 1) products in Fr — the points enter as PLAIN words, so both running products carry the same
//     power of 2^-256, which the quotient cancels — and one inversion (th_lagrange_*).  x_k - x_j is negative half the time and is
//     reduced into [0, r); it is never zero for distinct points below 2^33.
//   * TERM AND SUM: k_s P_s by the endomorphism ladder into a Jacobian scratch entry per term (msm_term), then a sum per segment in the
//     collect's two layouts: a lane walks a short segment in order, the lanes of a wave take the terms l, l + 64, .. of a long one and a
//     tree of six levels folds their partial sums (msm_lane_sum, msm_wave_partial, msm_tree_level over cl_tree_level).  Statuses follow
//     bn254_batch_g1_sum: the first non-zero decode status in segment order wins — in the wave layout the lowest index, carried beside it.
//   * OPTIMISTIC (bn254_batch_threshold_combine_keyed_optimistic): candidate rows, the settle that picks S' before any pairing, and the gates
//     of the two interpolations (tho_*, below rank and select).
// Include after bn254_collect.h and bn254_fr.h.
#pragma once

namespace bn254 {

// ---- rank and select ---------------------------------------------------------------------------------------------------------------------------
BN_DEV uint32_t th_popcount(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
BN_DEV uint32_t th_row_count(const uint32_t* row, size_t bm_words) {
  uint32_t n = 0;
  for (size_t w = 0; w < bm_words; ++w) n += th_popcount(row[w]);
  return n;
}
BN_DEV bool th_bit(const uint32_t* row, size_t bm_words, uint32_t key) {
  return (size_t)(key >> 5) < bm_words && ((row[key >> 5] >> (key & 31u)) & 1u) != 0;
}
// the row cut down to its t lowest bits (every bit of rank >= t cleared); a row of at most t bits stays as it is
BN_DEV void th_trim(uint32_t* row, size_t bm_words, uint32_t t) {
  uint32_t seen = 0;
  for (size_t w = 0; w < bm_words; ++w) {
    uint32_t v = row[w];
    const uint32_t pc = th_popcount(v);
    if (pc <= t - seen) { seen += pc; continue; }
    uint32_t kept = 0;
    for (uint32_t k = seen; k < t; ++k) { const uint32_t low = v & (0u - v); kept |= low; v ^= low; }
    row[w] = kept;
    seen = t;
  }
}
// one tuple behind the collect: status 0 and row V in, the verdict out.  |V| >= t: the row becomes S (exactly t bits), status stays 0;
// else the row stays V, the status reads VerificationFailed and the signature is the identity.  A tuple whose status is non-zero already
// (range rule, hash) has the empty row and the identity from the collect: nothing to do.  Returns |V|.
BN_DEV uint32_t th_settle(uint32_t* row, size_t bm_words, uint32_t t, uint8_t& tuple_st, uint8_t* sig64) {
  if (tuple_st != ST_OK) return 0;
  const uint32_t count = th_row_count(row, bm_words);
  if (count >= t) { th_trim(row, bm_words, t); return count; }
  tuple_st = ST_VERIFICATION_FAILED;
  uint32_t* w = (uint32_t*)sig64;
  for (int k = 0; k < 16; ++k) w[k] = 0;
  return count;
}
// is share s of tuple t (n: of nobody) the ONE summand of its key: the tuple combines, the share verified, its key's bit is in S, and this
// share is the first to claim it in the zeroed second row
BN_DEV bool th_take(const ClShares& in, uint64_t s, size_t t, size_t n, const uint32_t* used, uint32_t* claim, size_t bm_words) {
  if (t >= n || in.tuple_st[t] != ST_OK || in.share_st[s] != ST_OK) return false;
  const uint32_t key = in.key[s];
  if (!th_bit(used + t * bm_words, bm_words, key)) return false;
  return cl_claim(claim + t * bm_words, bm_words, key);
}

// ---- the optimistic call (bn254_batch_threshold_combine_keyed_optimistic[_device]) ----------------------------------------------------------------
// Interpolate first, verify the result once per tuple under the GROUP key.  The flags and the verdicts are the optimistic collect's
// (bn254_collect.h: CLO_FINAL / CLO_CHECK / CLO_EXACT, clo_goes_exact, clo_queued), so its queue and its counters serve this call as they stand.
//   * CANDIDATE ROW: a share whose pre-check status is 0 claims its key's bit in the tuple's output row; a refused claim is a second
//     candidate of one key and raises the tuple's duplicate byte (tho_candidate).  No sum: the row is all the first pass needs.
//   * SETTLE: a tuple whose status is non-zero already is final (empty row, identity, count 0); one with a duplicate or with fewer than t
//     candidates goes the exact way; else the row is cut down to S' = its t lowest bits and the tuple will be checked (tho_settle).
//   * SECOND PASS, for the tuples that go the exact way only: their rows are zeroed, their candidates verified, the status-0 shares claim
//     again (tho_reclaims) and th_settle runs as in the exact call (tho_resettle).  The byte it returns gates the second interpolation:
//     0 = this tuple combines now, anything else = its outputs stand (a tuple that passed, a final one, or one that just failed).
BN_DEV void tho_candidate(uint32_t* row, size_t bm_words, uint32_t key, uint8_t* dup) {
  if (!cl_claim(row, bm_words, key)) *dup = 1;
}
// one tuple behind the candidate rows: its flag; the row becomes S' iff the flag is CLO_CHECK.  sig64 is zeroed unless the tuple will be
// checked (the interpolation then writes it), so the tuple check decodes no byte the call has not written.  count = |C|, 0 for a final tuple.
BN_DEV uint8_t tho_settle(uint32_t* row, size_t bm_words, uint32_t t, uint8_t tuple_st, uint8_t dup, uint8_t* sig64, uint32_t& count) {
  uint8_t flag = CLO_FINAL;
  count = 0;
  if (tuple_st == ST_OK) {
    count = th_row_count(row, bm_words);
    flag = (dup || count < t) ? CLO_EXACT : CLO_CHECK;
  }
  if (flag == CLO_CHECK) { th_trim(row, bm_words, t); return flag; }
  uint32_t* w = (uint32_t*)sig64;
  for (int k = 0; k < 16; ++k) w[k] = 0;
  return flag;
}
// the first interpolation's gate (MSM_SEG_MASKED below: any non-zero byte masks): only the tuples that will be checked
BN_DEV uint8_t tho_gate(uint8_t flag) { return flag == CLO_CHECK ? (uint8_t)ST_OK : (uint8_t)0xFF; }
// does share s — status share_st behind the exact verify of the queue, of tuple t (n: of nobody) — claim its key in the second pass
BN_DEV bool tho_reclaims(uint8_t share_st, size_t t, size_t n, const uint8_t* flag, const uint8_t* verdict) {
  return clo_queued(share_st, t, n, flag, verdict);
}
// one tuple behind the second claim pass: a tuple that goes the exact way is settled as the exact call settles it (row V in; status, row,
// signature and count out); every other tuple is left alone.  Returns the second interpolation's gate.
BN_DEV uint8_t tho_resettle(uint32_t* row, size_t bm_words, uint32_t t, uint8_t flag, uint8_t verdict, uint8_t& tuple_st, uint8_t* sig64, uint32_t& count,
                            bool& mine) {
  mine = clo_goes_exact(flag, verdict);
  if (!mine) return 0xFF;
  tuple_st = ST_OK;                                    // only an accepted tuple with hash status 0 is ever flagged CLO_CHECK or CLO_EXACT
  count = th_settle(row, bm_words, t, tuple_st, sig64);
  return tuple_st == ST_OK ? (uint8_t)ST_OK : (uint8_t)0xFF;
}

// ---- Lagrange coefficients at zero -------------------------------------------------------------------------------------------------------------
// one factor k != j: num *= x_k, den *= x_k - x_j mod r, the factors as plain words (x < 2^33)
BN_DEV void th_lagrange_step(Fr& num, Fr& den, uint64_t xk, uint64_t xj) {
  Fr a = fr_zero(), d = fr_zero();
  a.w[0] = (uint32_t)xk; a.w[1] = (uint32_t)(xk >> 32);
  const uint64_t diff = xk > xj ? xk - xj : xj - xk;
  d.w[0] = (uint32_t)diff; d.w[1] = (uint32_t)(diff >> 32);
  if (xk < xj) d = fr_neg(d);
  num = fr_mul(num, a);
  den = fr_mul(den, d);
}
// num = 2^256 prod x_k / 2^(256 f), den the same of the differences, f factors each: num / den in Montgomery form is lambda's.  A repeated
// point (den = 0) gives 0; the threshold call cannot produce one.
BN_DEV Fr th_lagrange_finish(const Fr& num, const Fr& den) { return fr_mul(num, fr_inv(den)); }
// the coefficient of point j of the m points x[0 .. m) given directly (bn254_debug_lagrange_at_zero)
BN_DEV Fr th_lagrange_points(const uint32_t* x, uint64_t m, uint64_t j) {
  Fr num = fr_one(), den = fr_one();
  for (uint64_t k = 0; k < m; ++k)
    if (k != j) th_lagrange_step(num, den, x[k], x[j]);
  return th_lagrange_finish(num, den);
}
// ... and of key `key` in the set S given as a bitmap row: x_k = k + 1
BN_DEV Fr th_lagrange_row(const uint32_t* row, size_t bm_words, uint32_t key) {
  Fr num = fr_one(), den = fr_one();
  for (size_t w = 0; w < bm_words; ++w) {
    uint32_t v = row[w];
    while (v) {
      const uint32_t b = (uint32_t)__builtin_ctz(v);
      v &= v - 1u;
      const uint64_t k = (uint64_t)w * 32u + b;
      if (k != key) th_lagrange_step(num, den, k + 1u, (uint64_t)key + 1u);
    }
  }
  return th_lagrange_finish(num, den);
}

// ---- the scalar-weighted sum: term and sum -------------------------------------------------------------------------------------------------------
// term s = k P: the ladder's Jacobian result and the point's decode status.  !take, or a point that does not decode: the identity (the
// ladder walks it under the generator's coordinates, so the wave stays convergent; an identity point returns the identity by itself).
BN_DEV void msm_term(G1Jac& out, uint8_t& st, const uint8_t* point64, const uint8_t* scalar32, bool reduce, bool take) {
  G1Affine p;
  st = ST_OK;
  if (take) st = decode_g1(p, point64, 0);
  if (!take || st != ST_OK) { p.x = fp_load_const(C_G1_GEN[0]); p.y = fp_load_const(C_G1_GEN[1]); p.inf = true; }
  uint32_t k[8];
  for (int i = 0; i < 8; ++i) k[i] = 0;
  if (take) scalar_from_be(k, scalar32, reduce);
  g1_mul_glv_full(out, p, k);
}
// the terms of segment i as the sum walks them.  gate: a non-zero byte masks the segment out (the threshold call's tuple statuses: such a
// tuple's outputs stand already); else a range that is reversed or runs past the m terms is refused: no terms, status IndexOutOfBounds.
#define MSM_SEG_MASKED 0xFF
BN_DEV uint64_t msm_seg_len(const uint64_t* seg, size_t i, uint64_t m, const uint8_t* gate, uint8_t& st) {
  st = ST_OK;
  if (gate && gate[i] != ST_OK) { st = MSM_SEG_MASKED; return 0; }
  if (seg[i] > seg[i + 1] || seg[i + 1] > m) { st = ST_INDEX_OOB; return 0; }
  return seg[i + 1] - seg[i];
}
// one step of either walk: term lo + k of a segment of len terms; `bad` = the index of the first term whose status is non-zero (its status
// in st), UINT64_MAX while there is none.  J: G1Jac here, G2Jac for the sum in G2 (bn254_dealing.h)
template <class J>
BN_DEV void msm_step(J& acc, uint8_t& st, uint64_t& bad, const J* terms, const uint8_t* term_st, uint64_t lo, uint64_t len, uint64_t k) {
  J t;
  jac_set_identity(t);
  if (k < len) {
    t = terms[lo + k];
    const uint8_t s = term_st[lo + k];
    if (s != ST_OK && k < bad) { bad = k; st = s; }
  }
  jac_add(acc, acc, t);
}
template <class J>
BN_DEV void msm_lane_sum(J& acc, uint8_t& st, const J* terms, const uint8_t* term_st, uint64_t lo, uint64_t len) {
  uint64_t bad = UINT64_MAX;
  jac_set_identity(acc);
  for (uint64_t k = 0; BN_WAVE_ANY(k < len); ++k) msm_step(acc, st, bad, terms, term_st, lo, len, k);
}
template <class J>
BN_DEV void msm_wave_partial(J& acc, uint8_t& st, uint64_t& bad, const J* terms, const uint8_t* term_st, uint64_t lo, uint64_t len, unsigned lane) {
  bad = UINT64_MAX;
  st = ST_OK;
  jac_set_identity(acc);
  for (uint64_t k = lane; BN_WAVE_ANY(k < len); k += BN_CL_WAVE) msm_step(acc, st, bad, terms, term_st, lo, len, k);
}
// one level of the collect's tree, the earliest bad term carried along (cnt: the collect's counters, here the lanes folded)
template <class Slot>
BN_DEV void msm_tree_level(Slot* part, uint32_t* cnt, uint8_t* st, uint64_t* bad, unsigned t, unsigned stride) {
  cl_tree_level(part, cnt, t, stride);
  if (bad[t + stride] < bad[t]) { bad[t] = bad[t + stride]; st[t] = st[t + stride]; }
}
// the sum as the caller gets it: the identity (64 zero bytes) under a non-zero status
BN_DEV void msm_encode(uint8_t* out64, const G1Jac& acc, uint8_t st) {
  G1Affine r;
  jac_to_affine(r, acc);
  if (st != ST_OK) r.inf = true;
  encode_g1(out64, r);
}

}  // namespace bn254
