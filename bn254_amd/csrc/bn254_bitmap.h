// Same-message aggregates given as SIGNER BITMAPS over the registered keys (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap[_device]):
// the arithmetic and the bit logic of the aggregate key  sum_{j set} pk_j, shared by the device kernels (bn254_bitmap.hip: table builder and
// the one-lane sum; bn254_bitmap_pair.hip: the sum on lane pairs) and their host compilation for the CPU suite (tests/hostsim, plain and
// under -DBN_TRACK_BOUNDS).  Written against the fp2_* interface and two accessors, so it compiles for both layouts of Fq2.
//   * SUBSET TABLES of the registered set ("four Russians", as k_pool_subsets_g2 for the pools of the aggregate verify): window w = the keys
//     8w .. 8w + 7, entry w * 256 + mask = the sum of the window's keys whose bit is set in mask — affine, with an identity flag.  A byte of
//     a bitmap IS such a mask: an aggregate key costs n_keys / 8 table additions instead of popcount key additions.  A refused key (status
//     != 0), a registered identity key and a key index >= n_keys count as the identity; the tuples that name a refused or missing key get
//     their status from rule 2 anyway.  Record = a G2 pool record (bn254_ws.h): [x.re | y.re | 2 pad] [x.im | y.im | 2 pad], 40 words, so
//     that a lane of the pair layout reads the half of its role; 161 B per entry, 5 152 B per registered key.
//   * the WALK: the bytes of a tuple's bitmap in ascending order, zero bytes skipped (a wave skips a position none of its lanes needs), one
//     complete addition per byte (jac_accumulate_from: doubling, opposite points, an identity accumulator and identity entries all resolve
//     inside it); without tables, the same walk bit by bit over key_xy.
//   * RULE 2: the status of the LOWEST set bit that names a missing (>= n_keys: 2, IndexOutOfBounds) or refused (its registration status)
//     key, from bits & (bad | out of range) word by word; `bad` = one bit per registered key, set where its status is non-zero.
// Include after bn254_pairing.h (either layout).
#pragma once

namespace bn254 {

#define BM_HALF_WORDS 20                   /* = BN_POOL_HALF_WORDS: x (9 words) | y (9) | 2 pad */
#define BM_REC_WORDS (2 * BM_HALF_WORDS)
#define BM_KEY_WORDS (4 * BN_LIMBS)        /* key_xy: x.re | x.im | y.re | y.im, as k_register_keys stores a key */
#define BM_TABLE_BYTES_PER_KEY ((size_t)256 * (BM_REC_WORDS * sizeof(int32_t) + 1) / 8)

// the registered set as registration leaves it (bn254_ctx: key_xy, key_st, key_inf) and its bad-bit vector
struct BmKeys { const int32_t* xy; const uint8_t* st; const uint8_t* inf; const uint32_t* bad; uint32_t n_keys; };
struct BmTable { int32_t* rec; uint8_t* inf; };

// Words in memory (key_xy, table records) are coordinates as the kernels left them: carried limbs, |value| <= q — the contract the bound
// tracker of the host compilation checks at every store of an entry and assumes at every load.
#define BM_WORD_VMAX 1.0
BN_DEV Fp bm_load_fp(const int32_t* w) {
  Fp r;
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) r.v[k] = w[k];
  BN_TRK(bn_set_tight(r, -BM_WORD_VMAX, BM_WORD_VMAX));
  return r;
}
BN_DEV void bm_store_fp(int32_t* w, const Fp& a) {
  BN_TRK(if (a.bd.lo < -BN_T || a.bd.hi > BN_T || a.bd.vlo < -BM_WORD_VMAX || a.bd.vhi > BM_WORD_VMAX) bn_bound_fail("table entry outside the stored-word contract", bn_vabs(a)));
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) w[k] = a.v[k];
}
#if defined(BN_SPLIT_FP2)
BN_DEV void bm_load_fp2(Fp2& r, const int32_t* re, const int32_t* im) { BN_FOR_ROLES(k) r.c[k] = bm_load_fp(bn_role_index(k) ? im : re); }
BN_DEV void bm_store_fp2(const Fp2& a, int32_t* re, int32_t* im) { BN_FOR_ROLES(k) bm_store_fp(bn_role_index(k) ? im : re, a.c[k]); }
#else
BN_DEV void bm_load_fp2(Fp2& r, const int32_t* re, const int32_t* im) { r.c0 = bm_load_fp(re); r.c1 = bm_load_fp(im); }
BN_DEV void bm_store_fp2(const Fp2& a, int32_t* re, int32_t* im) { bm_store_fp(re, a.c0); bm_store_fp(im, a.c1); }
#endif

// sources of an in-place addition (bn254_curve.h: jac_accumulate_from): pointer and flag travel in registers, the words are fetched inside
#if defined(__HIPCC__)
#define BM_MEMBER __device__ __forceinline__
#else
#define BM_MEMBER inline          /* BN_DEV is `static` on the host: not for a member */
#endif
struct BmRecSrc {
  const int32_t* p;
  bool inf;
  BM_MEMBER void operator()(G2Affine& q) const {
    bm_load_fp2(q.x, p, p + BM_HALF_WORDS);
    bm_load_fp2(q.y, p + BN_LIMBS, p + BM_HALF_WORDS + BN_LIMBS);
    q.inf = inf;
  }
};
struct BmKeySrc {
  const int32_t* p;
  bool inf;
  BM_MEMBER void operator()(G2Affine& q) const {
    bm_load_fp2(q.x, p, p + BN_LIMBS);
    bm_load_fp2(q.y, p + 2 * BN_LIMBS, p + 3 * BN_LIMBS);
    q.inf = inf;
  }
};
// key j as a summand: the identity when it is refused, a registered identity, out of range or not selected (its stored coordinates are
// then the generator's — never (0, 0))
BN_DEV BmKeySrc bm_key_src(const BmKeys& K, uint32_t j, bool selected) {
  const uint32_t jj = j < K.n_keys ? j : 0;
  return BmKeySrc{K.xy + (size_t)jj * BM_KEY_WORDS, !selected || j >= K.n_keys || K.st[jj] != 0 || K.inf[jj] != 0};
}

// ---- the table builder: one entry (needs n_keys > 0) --------------------------------------------------------------------------------------
// `live` = false computes with identities only (a lane past the end keeps the wave's votes company)
BN_DEV void bm_subset_entry(G2Affine& a, const BmKeys& K, uint32_t window, uint32_t mask, bool live) {
  G2Jac acc;
  jac_set_identity(acc);
  for (int b = 0; b < 8; ++b) {                      // wave-uniform: the additions vote across the wave
    G2Affine p;
    bm_key_src(K, window * 8 + (uint32_t)b, live && ((mask >> b) & 1u))(p);
    jac_accumulate(acc, p);
  }
  jac_to_affine(a, acc);
}
BN_DEV void bm_store_entry(const BmTable& T, size_t j, const G2Affine& a) {
  int32_t* r = T.rec + j * BM_REC_WORDS;
  bm_store_fp2(a.x, r, r + BM_HALF_WORDS);
  bm_store_fp2(a.y, r + BN_LIMBS, r + BM_HALF_WORDS + BN_LIMBS);
}
// word w of the bad-bit vector: bit b set where key 32 w + b was refused at registration
BN_DEV uint32_t bm_bad_word(const uint8_t* key_st, uint32_t n_keys, uint32_t w) {
  uint32_t r = 0;
  for (uint32_t b = 0; b < 32; ++b) {
    const uint32_t j = 32 * w + b;
    if (j < n_keys && key_st[j] != 0) r |= 1u << b;
  }
  return r;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------------
// row = the tuple's bm_words words (signer j = bit j % 32 of word j / 32); bm_words and K are the same for every lane of a wave, so the loop
// bounds are wave-uniform; a lane that is not live walks zeros.  Words past ceil(n_keys / 32) hold no key: rule 2 deals with them.
BN_DEV uint32_t bm_walk_words(size_t bm_words, uint32_t n_keys) {
  const size_t nw = ((size_t)n_keys + 31) / 32;
  return (uint32_t)(bm_words < nw ? bm_words : nw);
}
// with tables: byte b of the bitmap selects entry b * 256 + byte.  The first byte SEEDS the sum (a load; an addition to the identity would
// take the complete formula for the whole wave); a later addition to a still-empty sum takes that formula, which is right and rare.
BN_DEV void bm_sum_tables(G2Jac& acc, const uint32_t* row, size_t bm_words, bool live, const BmKeys& K, const int32_t* rec, const uint8_t* rec_inf) {
  const uint32_t nw = bm_walk_words(bm_words, K.n_keys), n_windows = (K.n_keys + 7) / 8;
  jac_set_identity(acc);
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t word = live ? row[w] : 0u;
    if (!BN_WAVE_ANY(word != 0)) continue;
    for (uint32_t k = 0; k < 4 && 4 * w + k < n_windows; ++k) {
      const uint32_t byte = (word >> (8 * k)) & 255u;
      if (!BN_WAVE_ANY(byte != 0)) continue;
      const size_t j = (size_t)(4 * w + k) * 256 + byte;
      const BmRecSrc src{rec + j * BM_REC_WORDS, byte == 0 || rec_inf[j] != 0};
      if (w == 0 && k == 0) { G2Affine e; src(e); jac_from_affine(acc, e); }
      else jac_accumulate_from(acc, src);
    }
  }
}
// without tables (key sets above BN254_OPT_BITMAP_TABLE_MAX_KEYS): key by key from key_xy, the same order and the same additions
BN_DEV void bm_sum_keys(G2Jac& acc, const uint32_t* row, size_t bm_words, bool live, const BmKeys& K) {
  const uint32_t nw = bm_walk_words(bm_words, K.n_keys);
  jac_set_identity(acc);
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t word = live ? row[w] : 0u;
    if (!BN_WAVE_ANY(word != 0)) continue;
    for (uint32_t b = 0; b < 32 && 32 * w + b < K.n_keys; ++b) {
      const bool sel = ((word >> b) & 1u) != 0;
      if (!BN_WAVE_ANY(sel)) continue;
      const BmKeySrc src = bm_key_src(K, 32 * w + b, sel);
      if (w == 0 && b == 0) { G2Affine e; src(e); jac_from_affine(acc, e); }
      else jac_accumulate_from(acc, src);
    }
  }
}
// the sum as the verify kernels read a public key: affine, the generator's coordinates under the identity flag (as a registered identity key)
BN_DEV void bm_sum_to_key(G2Affine& pk, const G2Jac& acc) {
  jac_to_affine(pk, acc);
  pk.x = fp2_select(pk.inf, fp2_load_const(C_G2_GEN[0]), pk.x);
  pk.y = fp2_select(pk.inf, fp2_load_const(C_G2_GEN[1]), pk.y);
}

// ---- rule 2 --------------------------------------------------------------------------------------------------------------------------------
// 0, or the status of the lowest set bit that is bad: 2 for a bit at or above n_keys, else the key's registration status
BN_DEV uint8_t bm_rule2_status(const uint32_t* row, size_t bm_words, const BmKeys& K) {
  const size_t nw = ((size_t)K.n_keys + 31) / 32;
  for (size_t w = 0; w < bm_words; ++w) {
    const uint32_t word = row[w];
    if (word == 0) continue;
    uint32_t b = word;
    if (w < nw) {
      const uint32_t rem = K.n_keys - (uint32_t)(32 * w);                        // keys of this word: 1 .. 32 of them exist
      b = word & (K.bad[w] | (rem >= 32 ? 0u : ~0u << rem));
    }
    if (b) {
      const size_t j = 32 * w + (size_t)__builtin_ctz(b);
      return j >= K.n_keys ? (uint8_t)ST_INDEX_OOB : K.st[j];
    }
  }
  return ST_OK;
}

}  // namespace bn254
