// The G1 side of the randomised batch verification of signer-bitmap aggregates (bn254_bitmap_rand.hip; include/bn254_hip.h:
// bn254_batch_verify_keyed_bitmap_randomized[_device]), as device functions: bucket numbering, the fold of a window's byte
// buckets into its eight key sums, and the places of a group's table pairs.  Include after bn254_curve.h.
//
// Tuple i of a slice belongs to GROUP i / G.  Window w = the keys 8w .. 8w + 7; byte w of a tuple's bitmap, v != 0, sends r_i H(m_i) into the
// BYTE BUCKET (g, w, v): one addition per non-zero byte whatever the popcount.  A group owns 255 buckets per window and one more for
// S_g = sum r_i sigma_i, numbered like the (group, key) buckets of bn254_aggrand.h with 255 * windows "keys", so that the counting sort and
// the segmented sums of that call serve this one unchanged.  The FOLD turns the 255 sums B[v] of a (g, w) into
//     T_{g, 8w + b} = sum_{v : bit b of v} B[v]
// by halving: T_7 is the sum of the upper half, then the upper half is added onto the lower half (the index loses its top bit) and the same
// is done for bit 6, .. 0 — 255 additions for the sums, 255 for the halvings, all complete (equal messages give equal or opposite points;
// an empty bucket is the identity like any other value).
#pragma once

#define BMR_WINDOW_BUCKETS 255u

struct BmrSlot { G1Jac v; int32_t pad; };            // an LDS slot of odd stride, as the randomised verify's

BN_DEV uint32_t bmr_windows(uint32_t n_keys) { return (n_keys + 7u) / 8u; }
BN_DEV uint32_t bmr_virtual_keys(uint32_t n_keys) { return bmr_windows(n_keys) * BMR_WINDOW_BUCKETS; }   // the bucket behind them is S_g's
BN_DEV uint64_t bmr_bucket(uint64_t g, uint32_t w, uint32_t v, uint32_t n_keys) {                         // v = 1 .. 255
  return g * ((uint64_t)bmr_virtual_keys(n_keys) + 1) + (uint64_t)w * BMR_WINDOW_BUCKETS + (v - 1u);
}
BN_DEV uint64_t bmr_sig_bucket(uint64_t g, uint32_t n_keys) { return g * ((uint64_t)bmr_virtual_keys(n_keys) + 1) + bmr_virtual_keys(n_keys); }
// byte w of a tuple's bitmap (0 past its words)
BN_DEV uint32_t bmr_byte(const uint32_t* row, size_t bm_words, uint32_t w) { return (size_t)(w >> 2) < bm_words ? (row[w >> 2] >> (8u * (w & 3u))) & 255u : 0u; }

// the keys of window w that can carry a table pair: registered, accepted, not the identity
BN_DEV uint32_t bmr_window_keys(uint32_t w, uint32_t n_keys, const uint8_t* key_st, const uint8_t* key_inf) {
  uint32_t m = 0;
  for (uint32_t b = 0; b < 8; ++b) {
    const uint32_t j = 8u * w + b;
    if (j < n_keys && key_st[j] == 0 && key_inf[j] == 0) m |= 1u << b;
  }
  return m;
}
// the rank of key 8w + b among the window's table pairs (mask = the keys with a contributor)
BN_DEV uint32_t bmr_pair_rank(uint32_t mask, uint32_t b) { return (uint32_t)__builtin_popcount(mask & ((1u << b) - 1u)); }

// One level of the fold for bit `bit` (h = 1 << bit), as three lane steps with a barrier between them; lane t of at least 128.
//   copy: R[t] = B[t + h];  down: B[t] += R[t];  tree (d = h / 2, .. 1): R[t] += R[t + d]  — afterwards R[0] = T_bit.
BN_DEV void bmr_fold_copy(BmrSlot* R, const BmrSlot* B, unsigned h, unsigned t) { if (t < h) R[t].v = B[t + h].v; }
BN_DEV void bmr_fold_down(BmrSlot* B, const BmrSlot* R, unsigned h, unsigned t) { if (t < h) jac_add(B[t].v, B[t].v, R[t].v); }
BN_DEV void bmr_fold_tree(BmrSlot* R, unsigned d, unsigned t) { if (t < d) jac_add(R[t].v, R[t].v, R[t + d].v); }
// The whole fold as PHASES with a barrier after each: bit 7 first, per bit copy, down, its `bit` tree rounds, then lane 0 keeps R[0] as
// T[bit].  B = 256 slots (B[0] the identity), R = 128, T = 8; every lane 0 .. 255 calls every phase (k_bmr_fold: a workgroup; the host
// compilation: lane after lane).
#define BMR_FOLD_PHASES 52                           /* sum over bit = 7 .. 0 of 3 + bit */
BN_DEV void bmr_fold_phase(BmrSlot* B, BmrSlot* R, BmrSlot* T, int phase, unsigned t) {
  int bit = 7;
  while (phase >= 3 + bit) { phase -= 3 + bit; --bit; }
  const unsigned h = 1u << bit;
  if (phase == 0) bmr_fold_copy(R, B, h, t);
  else if (phase == 1) bmr_fold_down(B, R, h, t);
  else if (phase <= 1 + bit) bmr_fold_tree(R, h >> (phase - 1), t);
  else if (t == 0) T[bit].v = R[0].v;
}
