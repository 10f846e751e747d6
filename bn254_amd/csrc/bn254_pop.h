// Proofs of possession (include/bn254_hip.h: bn254_batch_pop_prove / _verify, bn254_ctx_register_keys_pop): the front end of the calls' own
// kernels (bn254_pop.hip), shared with their host compilation for the CPU suite (tests/hostsim).  The pairing work of a proof
// is a verify of the message TAG || pk — the existing verify, sign and keyed routes; what is new is written here:
//   * the COMPOSER: from n keys (128 B each, as the caller passed them) the n proof messages BN254_POP_TAG || pk_j, 144 B each, back to back,
//     the n + 1 offsets 144 j of the message arrays, and — for a registration — key_idx[j] = j.  A byte mover: element t of the launch is WORD
//     t of the message buffer (36 words per message: 4 of the tag, 32 of the key), so lane i of a wave stores the word at base + 4 i and,
//     inside a key, loads the word at base' + 4 i — both coalesced, one word per lane.  Keys and messages are 4-byte aligned (the staging
//     slots and the context's buffer are; the _device forms ask it of the caller), 144 = 36 x 4.
//   * the FOLD of two status arrays, first[j] ? first[j] : second[j] — a registration status in front of the proof's, the key derivation's
//     in front of the signature's.  One byte per lane, consecutive lanes consecutive bytes.
// Nothing here touches a field element: the header needs no other header of the library.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/bn254_hip.h"

#if defined(__HIPCC__)
#define BN_POP_DEV __host__ __device__ __forceinline__   /* the launchers size their grids by pop_compose_elems */
#else
#define BN_POP_DEV static inline
#endif

namespace bn254 {

#define BN_POP_KEY_WORDS 32                                      /* an uncompressed G2 point */
#define BN_POP_TAG_WORDS (BN254_POP_TAG_LEN / 4)
#define BN_POP_MSG_WORDS (BN_POP_TAG_WORDS + BN_POP_KEY_WORDS)   /* 36 */
#define BN_POP_MSG_BYTES (4 * BN_POP_MSG_WORDS)                  /* 144 */
static_assert(BN254_POP_TAG_LEN % 4 == 0 && sizeof(BN254_POP_TAG) == BN254_POP_TAG_LEN + 1, "the tag is whole words, and as long as the header says");

// what the composer writes for n keys: msgs 36 n words, off n + 1 entries, key_idx n entries (may be null: the prove and verify calls)
struct PopMsgs { uint32_t* msgs; uint64_t* off; uint32_t* key_idx; };

// elements of a launch over n keys: one per message word, and at least the n + 1 offsets (n = 0: the one offset)
BN_POP_DEV size_t pop_compose_elems(size_t n) { return n ? n * BN_POP_MSG_WORDS : 1; }

// word k of the tag as it lies in memory (the library's targets and hosts are little-endian: byte 4 k is the low one)
BN_POP_DEV uint32_t pop_tag_word(unsigned k) {
  const char tag[] = BN254_POP_TAG;
  return (uint32_t)(uint8_t)tag[4 * k] | (uint32_t)(uint8_t)tag[4 * k + 1] << 8 | (uint32_t)(uint8_t)tag[4 * k + 2] << 16 | (uint32_t)(uint8_t)tag[4 * k + 3] << 24;
}

// element t of the composer: word t of the messages (t < 36 n), offset t (t <= n), key index t (t < n)
BN_POP_DEV void pop_compose_elem(size_t t, size_t n, const uint32_t* pks, const PopMsgs& out) {
  if (t < n * BN_POP_MSG_WORDS) {
    const size_t j = t / BN_POP_MSG_WORDS;
    const unsigned k = (unsigned)(t % BN_POP_MSG_WORDS);
    out.msgs[t] = k < BN_POP_TAG_WORDS ? pop_tag_word(k) : pks[j * BN_POP_KEY_WORDS + (k - BN_POP_TAG_WORDS)];
  }
  if (t <= n) out.off[t] = (uint64_t)t * BN_POP_MSG_BYTES;
  if (t < n && out.key_idx) out.key_idx[t] = (uint32_t)t;
}

// the fold: the first status wins unless it is 0
BN_POP_DEV uint8_t pop_fold(uint8_t first, uint8_t second) { return first ? first : second; }
BN_POP_DEV void pop_fold_elem(size_t j, size_t n, uint8_t* first, const uint8_t* second) {
  if (j < n) first[j] = pop_fold(first[j], second[j]);
}

}  // namespace bn254
