// What the signer-bitmap calls RETURN besides a status byte (include/bn254_hip.h: bn254_batch_aggregate_keys_bitmap[_device],
// bn254_batch_verify_keyed_bitmap_export[_device], bn254_batch_bitmap_weights[_device]): the per-item bodies of the kernels of
// bn254_bitmap_out.hip, shared with their host compilation for the CPU suite (tests/hostsim: a stand-alone program, plain, under sanitizers
// and under -DBN_TRACK_BOUNDS).  Written against Fp alone — a coordinate of Fq2 is handed over as its two Fp halves — so the same text
// compiles under both layouts of Fq2 and on the host.  Include after bn254_pairing.h (either layout) and bn254_bitmap.h.
//   * EMIT: the aggregate key of workspace entry i (the Q planes as k_bm_sum / k_bm_sum_pair left them: affine, the generator's coordinates
//     under the identity flag) and H(m_i) (the P2 planes) as the reference's uncompressed bytes — 128 and 64 bytes, all zero for the
//     identity and for an entry whose status so far is not 0.  No inversion: bm_sum_to_key has paid it.
//   * SETTLE, behind the verify: the outputs of a tuple whose FINAL status is neither 0 nor 9 are zeroed (rules 1-3 did not all pass).
//   * WEIGHTS: byte-indexed tables of u64 subset sums of the registered keys' weights (window w = keys 8w .. 8w + 7, entry w * 256 + mask,
//     2 KB per 8 keys) — a byte of a bitmap is one lookup, n_keys / 8 lookups a tuple.  The total of all weights is < 2^64 (checked where
//     they are set), so no subset sum wraps.
// The outputs are written as 32-bit words and must be 4-byte aligned.
#pragma once

namespace bn254 {

BN_DEV void bmo_fp_to_be(uint8_t* p, const Fp& a) {
  const U256 t = fp_to_u256(a);
  uint32_t* w = (uint32_t*)p;
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = __builtin_bswap32(t.w[7 - i]);
}
BN_DEV void bmo_zero(uint8_t* p, int words) {
  uint32_t* w = (uint32_t*)p;
  for (int i = 0; i < words; ++i) w[i] = 0;
}
// item of the emit kernel, key half: x = (x_re, x_im), y = (y_re, y_im) -> x.re || x.im || y.re || y.im
BN_DEV void bmo_emit_key(uint8_t* out128, const Fp& x_re, const Fp& x_im, const Fp& y_re, const Fp& y_im, bool inf, uint8_t status) {
  if (inf || status != ST_OK) { bmo_zero(out128, 32); return; }
  bmo_fp_to_be(out128, x_re); bmo_fp_to_be(out128 + 32, x_im); bmo_fp_to_be(out128 + 64, y_re); bmo_fp_to_be(out128 + 96, y_im);
}
// ... hash half: the bytes bn254_batch_hash_to_g1 writes for the message
BN_DEV void bmo_emit_hash(uint8_t* out64, const Fp& x, const Fp& y, bool inf, uint8_t status) {
  if (inf || status != ST_OK) { bmo_zero(out64, 16); return; }
  bmo_fp_to_be(out64, x); bmo_fp_to_be(out64 + 32, y);
}
// item of the settle kernel: a tuple keeps its outputs iff it passed rules 1-3, i.e. its final status is 0 or 9
BN_DEV bool bmo_keeps(uint8_t final_status) { return final_status == ST_OK || final_status == ST_VERIFICATION_FAILED; }
BN_DEV void bmo_settle_item(uint8_t final_status, uint8_t* hash64 /* or null */, uint8_t* key128 /* or null */) {
  if (bmo_keeps(final_status)) return;
  if (hash64) bmo_zero(hash64, 16);
  if (key128) bmo_zero(key128, 32);
}

// ---- weights -------------------------------------------------------------------------------------------------------------------------------
#define BMW_WINDOW_ENTRIES 256
// entry window * 256 + mask of the weight tables: the weights of the window's keys whose bit is set in mask (keys at or above n_keys: 0)
BN_DEV uint64_t bmw_subset_entry(const uint64_t* weights, uint32_t n_keys, uint32_t window, uint32_t mask) {
  uint64_t s = 0;
  for (uint32_t b = 0; b < 8; ++b) {
    const uint32_t j = window * 8 + b;
    if (j < n_keys && ((mask >> b) & 1u)) s += weights[j];
  }
  return s;
}
// item of the weight kernel: the weight of one row from the tables (the words that hold a registered key: bm_walk_words) — what the call
// returns where rule 2 gives 0; a refused key's and an out-of-range bit's tuple has a non-zero status and weight 0
BN_DEV uint64_t bmw_row_weight(const uint32_t* row, size_t bm_words, uint32_t n_keys, const uint64_t* tab) {
  const uint32_t nw = bm_walk_words(bm_words, n_keys), n_windows = (n_keys + 7) / 8;
  uint64_t s = 0;
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t word = row[w];
    if (word == 0) continue;
    for (uint32_t k = 0; k < 4 && 4 * w + k < n_windows; ++k) s += tab[(size_t)(4 * w + k) * BMW_WINDOW_ENTRIES + ((word >> (8 * k)) & 255u)];
  }
  return s;
}
BN_DEV void bmw_item(const uint32_t* row, size_t bm_words, const BmKeys& K, const uint64_t* tab, uint64_t& weight, uint8_t& status) {
  status = bm_rule2_status(row, bm_words, K);
  weight = status == ST_OK ? bmw_row_weight(row, bm_words, K.n_keys, tab) : 0;
}

}  // namespace bn254
