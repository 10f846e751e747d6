/*
 * bn254_hip.h — C ABI of libbn254hip.so, the MI355X (gfx950) batch BN254 aggregate-signature
 * verifier.  This is the drop-in boundary: plain pointers and sizes, no HIP/torch types.
 *
 * The reference (sedaprotocol/bn254, a pure-Rust crate) has no FFI; its only boundary is the
 * Rust API re-exported at /root/reference/src/lib.rs:60-63.  Each entry point below states the
 * reference function whose per-item semantics it reproduces; INTEGRATION.md shows the Rust
 * `extern "C"` block + `ECDSA::batch_verify` shim a maintainer would add.
 *
 * Byte formats (the reference's *uncompressed* encodings):
 *   G1 point  : 64 bytes  x || y                       big-endian   (src/utils.rs:182-194)
 *   G2 point  : 128 bytes x.re || x.im || y.re || y.im big-endian   (src/utils.rs:161-179)
 *   scalar    : 32 bytes big-endian
 *   Gt        : 384 bytes, 12 x BE32 in tower order (Fq12 = Fq6[w]/(w^2-v), Fq6 = Fq2[v]/(v^3-xi)):
 *               a0.re a0.im a1.re a1.im a2.re a2.im b0.re ... b2.im  (build-defined: the reference
 *               never serialises Gt, src/lib.rs:60-63)
 *   identity  : all-zero bytes (the reference's typed API can hold it but to_uncompressed cannot
 *               encode it — PointInJacobian, src/utils.rs:163,184)
 *   messages  : one concatenated byte buffer + n+1 offsets (msg i = msgs[off[i] .. off[i+1]))
 *
 * Per-item status byte: 0 = Ok, otherwise 1 + the index of the reference's Error variant
 * (src/error.rs:6-29):  1 HashToPointError, 2 IndexOutOfBounds, 3 InvalidEncoding,
 * 4 InvalidGroupPoint, 5 InvalidLength, 6 NotMemberError, 7 ToAffineConversion, 8 PointInJacobian,
 * 9 VerificationFailed, 10 SerializationError, 11 HexDecodeFailed.
 *
 * Return value of every call: 0 on success (bad *items* only set their status byte),
 * -(hipError_t) for a HIP runtime failure, BN254_E_* for bad arguments.
 *
 * Ownership/threading: the caller owns every buffer; the library keeps no pointer after a
 * host-pointer call returns: such a call returns only after every copy from and to the caller's
 * buffers has finished, also when it fails.  A bn254_ctx is used by one thread at a time; distinct contexts
 * (distinct devices) are fully concurrent.  There is NO CPU fallback: every entry point runs
 * HIP kernels on the context's device and fails if that is impossible.
 *
 * *_device variants take DEVICE pointers (4-byte aligned, resident in HBM), enqueue on `stream`
 * (a hipStream_t passed as void*) and do not synchronise.  stream = NULL means the context's OWN stream, which is
 * created non-blocking: it has NO implicit ordering with the legacy null stream or any other stream, so a caller
 * that fills the inputs or reads the outputs on another stream must pass that stream (or order the two with events /
 * bn254_ctx_synchronize).  A context carries ONE call in flight: its workspace in HBM is shared by all its calls,
 * so a second *_device call may be enqueued only on the same stream as the first (stream order then keeps them
 * apart) — for concurrent calls on several streams create one context per stream.
 * Offsets arrays (n + 1 entries) must be non-decreasing: the host-pointer entry points check it and return
 * BN254_E_BAD_ARGUMENT.  The *_device variants cannot read their arrays on the host; the kernels check every pair
 * themselves: a message whose offsets are reversed — or, when the caller has declared the size of the message buffer
 * with bn254_ctx_expect_msgs_len, run past it — is never dereferenced and its item reports 5 (InvalidLength); the other
 * items of the batch are unaffected.
 */
#ifndef BN254_HIP_H
#define BN254_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bn254_ctx bn254_ctx;

#define BN254_FLAG_G2_SUBGROUP_CHECK 1u /* decode G2 inputs with the order-r check AffineG2::new performs */
#define BN254_FLAG_REJECT_IDENTITY 2u   /* treat all-zero encodings as InvalidGroupPoint (from_uncompressed behaviour) */
#define BN254_FLAG_G1_COMPRESSED 4u     /* the call's G1 INPUT array holds 33-byte compressed points (0x02 / 0x03 || x, Signature::from_compressed:
                                           src/serde.rs:39, src/utils.rs:84-104) and needs no alignment, also in the _device forms.  Every other
                                           array and every output is unchanged; aggregates the library WRITES stay 64 bytes (the identity is a
                                           legitimate aggregate and has no compressed form).  Taken, in the host-pointer and the _device form, by:
                                             bn254_batch_verify_keyed, bn254_batch_verify_keyed_randomized                        (sigs),
                                             bn254_batch_verify_keyed_bitmap, bn254_batch_verify_keyed_bitmap_randomized          (sigs),
                                             bn254_batch_collect_keyed_bitmap, its _randomized and its _optimistic form           (shares),
                                             bn254_batch_merge_keyed_bitmap and its _optimistic form                              (parts),
                                             bn254_batch_threshold_combine_keyed and its _optimistic form                         (shares).
                                           Every other entry point that reads 64-byte G1 points under a flags argument returns
                                           BN254_E_BAD_ARGUMENT when the bit is set (verify, verify_randomized, the aggregate and distinct-message
                                           families, the pairing and public-key checks, the pop calls, the multi-GPU layer): no call reads 33-byte
                                           data at a 64-byte stride.  Under the flag the array holds fewer than 2^32 items.
                                           THE DEFINING IDENTITY.  For an encoding c let (st, u) be what bn254_batch_g1_decompress returns for it
                                           (checks in the order documented there: x >= q gives 6, no square root gives 6, only then a bad prefix
                                           gives 3).  S(c) = u if st = 0, else the 64 bytes BE32(q) || 0..0, a stand-in whose decode status is 6
                                           under every flags value.  A call with the flag returns, byte for byte, what the same call without the
                                           flag returns on the items S(c) — with one change: an item with st != 0 whose status byte reads 6 in that
                                           run reports st instead.  (That byte is necessarily the item's own decode status: decode is the first
                                           rule everywhere, and the one thing that can precede it, the fill with 2 of an item of no accepted
                                           tuple, keeps reading 2.)  So such an item is never verified, taken, counted or made a candidate; the
                                           rule orders, the optimistic and randomised fallbacks with their documented deviations, and the
                                           BN254_OPT_MAX_CHUNK slicing hold unchanged.  BN254_FLAG_REJECT_IDENTITY has nothing to act on in the
                                           compressed array (no encoding decompresses to the identity).  The decompression runs once per call, on
                                           the device, in front of the call's first profiling event.  WHICH CALL WHEN: whoever holds compressed
                                           signatures passes them with this flag — measured (whole host-pointer calls) it
                                           is faster than decompressing through bn254_batch_g1_decompress and calling without the flag at every
                                           shape tried (by 0.14 ms at 43 776 shares to 1.4 ms at 350 208), and 0.11 to 0.6 ms slower than the
                                           same call on points that are ALREADY uncompressed: who holds those passes those. */
#define BN254_FLAG_RAND64 0x100u        /* bn254_batch_verify_randomized: 64-bit instead of 128-bit random scalars */
#define BN254_FLAG_RAND_GLV 0x200u      /* ... : r_i = k1 + k2*lambda mod r with k1, k2 the two 64-bit halves of the 128 random bits
                                           (lambda = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd, the eigenvalue of
                                           (x, y) -> (beta x, y) on G1): still 2^128 distinct multipliers, 30 % cheaper to apply */

#define BN254_E_BAD_ARGUMENT (-10001)
#define BN254_E_MISALIGNED (-10002)
#define BN254_E_NO_DEVICE (-10003)
#define BN254_E_RCCL (-10004)      /* multi-GPU layer: librccl.so.1 could not be loaded, or an RCCL call failed (bn254_mgpu_last_error has the text) */
#define BN254_E_NO_MEMORY (-10005) /* host allocation or thread creation failed */

/* status codes */
#define BN254_OK 0
#define BN254_ERR_HASH_TO_POINT 1
#define BN254_ERR_INDEX_OUT_OF_BOUNDS 2 /* keyed verify: key_idx >= n_keys; aggregate verify: signer / message index out of range */
#define BN254_ERR_INVALID_ENCODING 3
#define BN254_ERR_INVALID_GROUP_POINT 4
#define BN254_ERR_INVALID_LENGTH 5
#define BN254_ERR_NOT_MEMBER 6
#define BN254_ERR_TO_AFFINE_CONVERSION 7 /* never produced by the library (host mirrors: the reference's vocabulary, src/error.rs:6-29) */
#define BN254_ERR_POINT_IN_JACOBIAN 8
#define BN254_ERR_VERIFICATION_FAILED 9
#define BN254_ERR_SERIALIZATION 10       /* host mirrors only */
#define BN254_ERR_HEX_DECODE_FAILED 11   /* host mirrors only */

const char *bn254_version(void);

/* opaque context: device id, stream, workspace in HBM (grown on demand, reused across calls) */
int bn254_ctx_create(int hip_device, bn254_ctx **out);
void bn254_ctx_destroy(bn254_ctx *ctx);
/* pre-size the HBM workspace for batches of up to n items / n*k pairs (optional; avoids a
 * hipMalloc inside a later *_device call) */
int bn254_ctx_reserve(bn254_ctx *ctx, size_t n_items);
/* the same for the HOST-pointer bn254_batch_verify: workspace plus the staging buffers in HBM for n_items tuples whose messages total
 * msg_bytes, so that the steady state allocates nothing.  (Whenever a call does have to grow a buffer it first waits for the context's
 * own streams and for the stream of the context's last *_device call — not for the whole device.) */
int bn254_ctx_reserve_host(bn254_ctx *ctx, size_t n_items, size_t msg_bytes);
int bn254_ctx_synchronize(bn254_ctx *ctx);
/* Declares the size in bytes of the d_msgs buffer of the NEXT call on this context that hashes messages (verify, verify_compressed,
 * verify_randomized, hash_to_g1, sign, aggregate_verify and their *_device forms); the declaration is consumed by that call.
 * With it every message span is bounds-checked on the device (offsets non-decreasing and <= msgs_len), without it only
 * reversed offset pairs can be detected.  No counterpart in the reference: a Rust slice (src/ecdsa.rs:49) carries its length. */
int bn254_ctx_expect_msgs_len(bn254_ctx *ctx, uint64_t msgs_len);

/* Message arrays, in every call that takes msgs / msg_off: message i is the bytes msgs[msg_off[i] .. msg_off[i+1]), of any length
 * (an empty message is msg_off[i] == msg_off[i+1]); msg_off has n + 1 non-decreasing entries.  msg_off[0] need NOT be 0: the bytes
 * in front of it belong to no message and are never hashed.  The HOST forms nevertheless stage msgs[0 .. msg_off[n]) as a whole
 * (a call that slices its batch: each slice's own bytes) — so msgs must be readable from its first byte, and a large msg_off[0]
 * costs staging memory and copy time; pass msgs + msg_off[0] with rebased offsets to avoid both.  The *_device forms read message bytes only.
 * (tests/hash_cases.py, tests/test_gpu_hash_cases.py: every length 0 .. 200, the block edges of the SHA-256 padding, up to
 * 2^20 + 1 bytes, offsets behind a junk prefix.) */

/* status[i] = what ECDSA::verify(msg_i, sig_i, pk_i) returns (src/ecdsa.rs:49-64):
 * e(H(m), pk) * e(sig, -G2::one()) == 1.  Decoding errors of sig (first) or pk are reported with
 * the code from_uncompressed would give (src/utils.rs:107-127). */
int bn254_batch_verify(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */, const uint8_t *sigs /* n*64 */,
                       const uint8_t *pks /* n*128 */, size_t n, uint32_t flags, uint8_t *status /* n */);
int bn254_batch_verify_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_sigs,
                              const uint8_t *d_pks, size_t n, uint32_t flags, uint8_t *d_status, void *stream);

/* bn254_batch_verify from the COMPRESSED encodings callers store (serde of the reference: src/serde.rs:39, :54):
 * sigs n*33 B = 0x02/0x03 || x (src/utils.rs:84-104; G1::from_compressed, src/types.rs:233-237), pks n*65 B =
 * 0x0a/0x0b || BE64(x.im*q + x.re) (src/utils.rs:130-158; G2::from_compressed, src/types.rs:91-93, which checks the
 * order-r subgroup).  status[i] = the error the reference's from_compressed would give for the signature, else for
 * the public key (3 InvalidEncoding, 6 NotMemberError), else what verify gives.  No alignment requirement on the
 * 33- / 65-byte arrays. */
int bn254_batch_verify_compressed(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs33,
                                  const uint8_t *pks65, size_t n, uint8_t *status);
int bn254_batch_verify_compressed_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                         const uint8_t *d_sigs33, const uint8_t *d_pks65, size_t n, uint8_t *d_status,
                                         void *stream);

/* Keyed verify — the same check for public keys REGISTERED with the context beforehand (a validator set).
 * The reference validates a PublicKey once, at construction (PublicKey::from_uncompressed, src/types.rs:96-99 ->
 * src/utils.rs:107-116), and every ECDSA::verify (src/ecdsa.rs:49-64) then repeats the key-dependent half of the Miller
 * loop; here registration also tabulates that half (the 87 line functions of the key, 12.5 KB per key in HBM) and a keyed
 * verify reads it back instead of recomputing it: about a quarter of the Miller loop's field products disappear.
 *
 * bn254_ctx_register_keys replaces the context's key set with `n_keys` uncompressed G2 points (n_keys * 128 bytes, host
 * memory).  key_status[j] (may be NULL) = what PublicKey::from_uncompressed reports for key j: 0, 6 (a coordinate >= q) or 4
 * (not on the curve / not in the order-r subgroup — the subgroup check ALWAYS runs here, as in AffineG2::new; flags: only
 * BN254_FLAG_REJECT_IDENTITY is looked at).  An all-zero key is the identity (its pair contributes 1).  The call
 * waits for the context's own streams and for the stream of its last *_device call before it touches the tables — a keyed
 * verify enqueued earlier has finished reading them (a context carries one call in flight) — and returns with the new set in
 * place; the same holds whenever a call has to grow the context's workspace or staging buffers (presize with bn254_ctx_reserve /
 * bn254_ctx_reserve_host to keep that out of the steady state).  Other contexts and streams are not waited for.
 *
 * bn254_batch_verify_keyed[_device]: as bn254_batch_verify with key_idx[i] (uint32) in place of the i-th public key.
 * status[i] = the signature's decode error, else 2 (IndexOutOfBounds) if key_idx[i] >= n_keys, else the key's registration
 * status, else what verify gives.  Same result bytes as bn254_batch_verify(flags | BN254_FLAG_G2_SUBGROUP_CHECK) on the
 * expanded keys.  Batches of up to BN254_OPT_LM_MAX_BATCH tuples run the lane machine's keyed form on the line tables (latency: no twist
 * point to walk), batches of up to BN254_OPT_TRIO_MAX_BATCH the small-batch kernels on the expanded keys; the line tables serve the larger
 * ones too (throughput). */
int bn254_ctx_register_keys(bn254_ctx *ctx, const uint8_t *pks /* n_keys*128 */, size_t n_keys, uint32_t flags, uint8_t *key_status /* n_keys or NULL */);
int bn254_batch_verify_keyed(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */, const uint8_t *sigs /* n*64 */,
                             const uint32_t *key_idx /* n */, size_t n, uint32_t flags, uint8_t *status /* n */);
int bn254_batch_verify_keyed_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_sigs,
                                    const uint32_t *d_key_idx, size_t n, uint32_t flags, uint8_t *d_status, void *stream);

/* Keyed randomised batch verification — OPT-IN, probabilistic, for REGISTERED keys.  Items that share a public key share the G2
 * argument of their pairings, so 64 of them are checked by ONE product  e(sum r_i H(m_i), pk) * e(sum r_i sig_i, -G2) == 1  (two
 * table-driven Miller loops and one final exponentiation per 64 items; per item the two scalar multiplications by r_i).  Items are
 * grouped by key on the device; r_i as in bn254_batch_verify_randomized (first 16 / 8 bytes of SHA-256(seed32 || le64(i)), same flags
 * BN254_FLAG_RAND64 / BN254_FLAG_RAND_GLV); the items of a failing group are re-checked one by one with the exact keyed kernels.
 * Same inputs and status bytes as bn254_batch_verify_keyed: a non-zero status is always the exact one, a zero is wrong with
 * probability <= 2^-128 (2^-64) per group for a fresh secret seed.  Batches below BN254_OPT_RAND_MIN_BATCH, and contexts without
 * registered keys, take the exact keyed path.  No counterpart in the reference (src/ecdsa.rs:49-64 verifies one tuple at a time). */
int bn254_batch_verify_keyed_randomized(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs,
                                        const uint32_t *key_idx, size_t n, uint32_t flags, const uint8_t *seed32, uint8_t *status);
int bn254_batch_verify_keyed_randomized_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_sigs,
                                               const uint32_t *d_key_idx, size_t n, uint32_t flags, const uint8_t *seed32,
                                               uint8_t *d_status, void *stream);

/* Randomised batch verification — OPT-IN, probabilistic.  No counterpart in the
 * reference, which verifies one tuple at a time (src/ecdsa.rs:49-64); same inputs and status bytes as
 * bn254_batch_verify.  Items are taken 64 at a time; with r_i = the first 16 bytes (BN254_FLAG_RAND64: 8) of
 * SHA-256(seed32 || le64(i)) read little-endian (0 -> 1; BN254_FLAG_RAND_GLV: see the flag), a group passes iff
 *     prod_i e(r_i * H(m_i), pk_i) * e(sum_i r_i * sig_i, -G2::one()) == 1      (over its items that decode and hash)
 * i.e. 64 + 1 Miller loops and ONE final exponentiation per 64 verifies.  Items of a passing group get status 0
 * (or their decode / hash error); every item of a failing group is re-verified exactly (the kernels of
 * bn254_batch_verify), so a non-zero status is always exact.  A zero status is wrong with probability <= 2^-128
 * (2^-64) per group PROVIDED seed32 is fresh, unpredictable to whoever produced the signatures, and the public
 * keys are in the order-r subgroup (validated earlier, or pass BN254_FLAG_G2_SUBGROUP_CHECK).  group_ok (optional,
 * ceil(n/64) bytes): 1 = the group's combined check passed.  The combined check has a fixed latency of one
 * Miller loop + one final exponentiation on n/64 lanes: it pays off from ~100 k items per call on an MI355X; smaller
 * batches are routed to the exact kernels (BN254_OPT_RAND_MIN_BATCH), see DESIGN.md.  Host variant synchronises; device variant only enqueues. */
int bn254_batch_verify_randomized(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs,
                                  const uint8_t *pks, size_t n, uint32_t flags, const uint8_t *seed32, uint8_t *status,
                                  uint8_t *group_ok);
int bn254_batch_verify_randomized_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                         const uint8_t *d_sigs, const uint8_t *d_pks, size_t n, uint32_t flags,
                                         const uint8_t *seed32 /* host memory */, uint8_t *d_status, uint8_t *d_group_ok,
                                         void *stream);

/* points[i] = hash_to_try_and_increment(msg_i) (src/hash.rs:29-63), uncompressed; status 1 =
 * HashToPointError; tries[i] (optional, may be NULL) = number of counters consumed (1..255). */
int bn254_batch_hash_to_g1(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, size_t n, uint8_t *points /* n*64 */,
                           uint8_t *status /* n */, uint8_t *tries /* n or NULL */);
int bn254_batch_hash_to_g1_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t n, uint8_t *d_points,
                                  uint8_t *d_status, uint8_t *d_tries, void *stream);

/* status[i] = (bn::pairing_batch(&[(g1[i*k+j], g2[i*k+j]); k]) == Gt::one()) ? 0 : 9 — the kernel
 * shared by ECDSA::verify and check_public_keys (src/ecdsa.rs:57-63, :86-92).
 *
 * The contract of the three pairing calls (tests/pairing_cases.py, tests/test_gpu_pairing.py):
 *   - Operands: all-zero bytes are the identity; a pair with an identity operand contributes one.  An item is decoded in the order
 *     g1[i*k], g2[i*k], g1[i*k+1], g2[i*k+1], ...: inside a pair G1 comes before G2, across the pairs of an item the lowest index comes
 *     first, and status[i] is the code of the FIRST operand in that order that does not decode (6 = a coordinate >= q; 4 = not on the
 *     curve / the twist, outside the subgroup under BN254_FLAG_G2_SUBGROUP_CHECK, an identity under BN254_FLAG_REJECT_IDENTITY).  Only
 *     when every operand decodes is it 0 / 9 by the product.  This is the order of the oracle's bn254o_batch_pairing.
 *   - k >= 1 has no upper bound of its own: a call needs workspace for n*k pairs (bn254_ctx_reserve's size, grown on demand; the
 *     call fails with the allocation's error when it cannot be had), and every route takes any k.  k == 0 is BN254_E_BAD_ARGUMENT.
 *   - gt[i] of an item whose status is a decode error is defined, and the same on every route: the product with the GENERATOR of its
 *     group (G1::one(), G2::one()) in place of every operand of the item that did not decode — all of them, not only the first — and
 *     the other operands as given.  It says nothing about the input; a caller reads status[i] first. */
int bn254_batch_pairing_check(bn254_ctx *ctx, const uint8_t *g1 /* n*k*64 */, const uint8_t *g2 /* n*k*128 */, size_t n, size_t k,
                              uint32_t flags, uint8_t *status /* n */);
/* gt[i] = prod_j e(g1[i*k+j], g2[i*k+j]) = Miller product ^ ((q^12-1)/r), 384 bytes each.  Batches that cannot fill the chip (n*k <=
 * BN254_OPT_LM_MAX_BATCH pairs, n <= 1024 items) take the small-batch kernels of a verify — the lane machine with the fixed pair skipped, the
 * exact final exponentiation on eighteen lane pairs per item: one pairing in 1.1 ms instead of 5.7; same bytes. */
int bn254_batch_pairing(bn254_ctx *ctx, const uint8_t *g1, const uint8_t *g2, size_t n, size_t k, uint32_t flags,
                        uint8_t *gt /* n*384 */, uint8_t *status /* n */);
int bn254_batch_pairing_device(bn254_ctx *ctx, const uint8_t *d_g1, const uint8_t *d_g2, size_t n, size_t k, uint32_t flags,
                               uint8_t *d_gt /* n*384 or NULL */, uint8_t *d_status, void *stream);

/* status[i] = check_public_keys(pk_g2[i], pk_g1[i]) (src/ecdsa.rs:78-93) */
int bn254_batch_check_public_keys(bn254_ctx *ctx, const uint8_t *pk_g2 /* n*128 */, const uint8_t *pk_g1 /* n*64 */, size_t n,
                                  uint32_t flags, uint8_t *status);

/* group operations: aggregation = `Add for Signature/PublicKey` (src/types.rs:126-132, :264-270),
 * sign / key derivation = G1*Fr, G2*Fr (src/ecdsa.rs:31, src/types.rs:86, :156).
 * reduce_scalar != 0: scalars are first reduced mod r like Fr::from_slice; 0: used as 256-bit integers.
 * p == NULL in the two _mul entry points multiplies the group's GENERATOR — key derivation, PublicKeyG1 / PublicKey::from_private_key
 * (src/types.rs:155-157, :85-87): a fixed base, served from a comb table of the generator's multiples built once per context (65 additions on a
 * lane pair instead of a 256-step ladder on one lane; window entries found by constant-time scans: the scalar is a private key).
 * With explicit G1 points, and in bn254_batch_sign, the multiplication runs a joint 128-step ladder over the curve's endomorphism
 * (k mod r = k1 + k2 lambda with 128-bit halves; every point of the G1 curve has order r, so a raw 256-bit scalar acts mod r — the same
 * point as the 256-step ladder gives); window entries by scans, complete additions. */
int bn254_batch_g1_add(bn254_ctx *ctx, const uint8_t *a /* n*64 */, const uint8_t *b /* n*64 */, size_t n, uint8_t *out, uint8_t *status);
int bn254_batch_g2_add(bn254_ctx *ctx, const uint8_t *a /* n*128 */, const uint8_t *b /* n*128 */, size_t n, uint8_t *out, uint8_t *status);
int bn254_batch_g1_mul(bn254_ctx *ctx, const uint8_t *p /* n*64 */, const uint8_t *scalars /* n*32 */, size_t n, int reduce_scalar,
                       uint8_t *out, uint8_t *status);
int bn254_batch_g2_mul(bn254_ctx *ctx, const uint8_t *p /* n*128 */, const uint8_t *scalars /* n*32 */, size_t n, int reduce_scalar,
                       uint8_t *out, uint8_t *status);
int bn254_batch_g1_mul_device(bn254_ctx *ctx, const uint8_t *d_p, const uint8_t *d_scalars, size_t n, int reduce_scalar,
                              uint8_t *d_out, uint8_t *d_status, void *stream);
int bn254_batch_g2_mul_device(bn254_ctx *ctx, const uint8_t *d_p, const uint8_t *d_scalars, size_t n, int reduce_scalar,
                              uint8_t *d_out, uint8_t *d_status, void *stream);
/* sigs[i] = ECDSA::sign(msg_i, sk_i) = H(msg_i) * sk_i (src/ecdsa.rs:26-35), uncompressed */
int bn254_batch_sign(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sks /* n*32 */, size_t n,
                     uint8_t *sigs /* n*64 */, uint8_t *status);
int bn254_batch_sign_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_sks, size_t n,
                            uint8_t *d_sigs, uint8_t *d_status, void *stream);
/* segmented aggregation: out[i] = sum of `counts[i]` consecutive points starting at points[first[i]]
 * (unit-scalar "MSM" of config 3: aggregate public key / aggregate signature) */
int bn254_batch_g1_sum(bn254_ctx *ctx, const uint8_t *points, const uint64_t *seg_off /* n+1 */, size_t n, uint8_t *out /* n*64 */, uint8_t *status);
int bn254_batch_g2_sum(bn254_ctx *ctx, const uint8_t *points, const uint64_t *seg_off /* n+1 */, size_t n, uint8_t *out /* n*128 */, uint8_t *status);
/* segmented SCALAR-WEIGHTED sum in G1: out[i] = sum over the terms s in [seg_off[i], seg_off[i+1]) of scalars[s] * points[s] — the sum of
 * bn254_batch_g1_sum with a scalar per point (interpolating threshold signatures, linear combinations of commitments).
 * DEFINING IDENTITY: byte for byte bn254_batch_g1_mul(points, scalars, reduce_scalar) followed by bn254_batch_g1_sum of the products over
 * the same segments.  reduce_scalar as in bn254_batch_g1_mul (a raw 256-bit scalar acts mod r on G1 either way).  Statuses follow
 * bn254_batch_g1_sum: the first non-zero decode status of a point in segment order wins, and the output is then the identity as 64 zero
 * bytes; an empty segment gives the identity with status 0; the identity (64 zero bytes) is a legal point.
 * Argument checks: n < 2^32, at most 2^32 - 1 terms; host form: seg_off non-decreasing (else BN254_E_BAD_ARGUMENT), points and scalars hold
 * seg_off[n] entries.  _device form: d_points, d_scalars and d_out 4-byte aligned, d_seg_off 8-byte aligned, else BN254_E_MISALIGNED; a
 * segment that is reversed or runs past d_seg_off[n] terms reads status 2 with the identity, never a read outside the buffers.  The number
 * of terms sizes the call's scratch (108 B per term), and the _device form learns it from d_seg_off[n]: ONE 8-byte copy to the host and a
 * wait for the stream before anything is enqueued — unlike the other _device forms it cannot be captured into a graph.  One call per
 * context in flight, as everywhere.
 * Cost: a term kernel, one lane per term (decode, the 128-step endomorphism ladder of bn254_batch_g1_mul, the Jacobian result to scratch —
 * no inversion per term), then one sum per segment in the two layouts of the collect: a lane per segment of fewer than
 * BN254_OPT_COLLECT_WAVE_MIN_SHARES terms, the 64 lanes of a wave with a six-level tree in LDS per longer one; one inversion per segment.
 * Measured on an MI355X (tools/threshold_throughput.py --msm, profiles/threshold_throughput.jsonl; 65 536 terms, host forms, median [min,
 * max] of 7): in 4 096 segments of 16 — the first length the wave layout takes — 3.48 ms [3.47, 3.53] against 3.23 [3.21, 3.26] for
 * bn254_batch_g1_mul + bn254_batch_g1_sum: 0.25 ms SLOWER; in one segment 14.8 ms [14.76, 14.87] against 766 [709, 865], where g1_sum walks
 * the segment in one lane.  The _device form: 3.30 and 14.70 ms.  Which call when: this one for long segments, or where the products are
 * not wanted; the two old calls for many segments of about 16.  The lane/wave split was not swept for this call.  DESIGN.md section 10k. */
int bn254_batch_g1_msm(bn254_ctx *ctx, const uint8_t *points /* m*64 */, const uint8_t *scalars /* m*32, big-endian */,
                       const uint64_t *seg_off /* n+1 */, size_t n, int reduce_scalar, uint8_t *out /* n*64 */, uint8_t *status /* n */);
int bn254_batch_g1_msm_device(bn254_ctx *ctx, const uint8_t *d_points, const uint8_t *d_scalars, const uint64_t *d_seg_off, size_t n,
                              int reduce_scalar, uint8_t *d_out, uint8_t *d_status, void *stream);
/* ... and in G2: out[i] = sum over the terms s in [seg_off[i], seg_off[i+1]) of scalars[s] * points[s], 128-byte points and outputs — the
 * building block for group keys (sum lambda_k pk_k), for linear combinations of commitments and for the dealing check below (a vector of
 * commitments at small integer points, sum x^k C_k, has a call of its own that needs no scalars: bn254_batch_g2_poly_eval).
 * Same argument list, argument checks, alignment rules and range rule of the _device form as bn254_batch_g1_msm above; the _device form makes
 * the same single 8-byte copy of d_seg_off[n] and so cannot be captured into a graph either.  Scratch: 217 B per term.
 * DEFINING IDENTITY: byte for byte bn254_batch_g2_mul(points, scalars, reduce_scalar) followed by bn254_batch_g2_sum of the products over
 * the same segments, the identity as 128 zero bytes included.  The first non-zero decode status in segment order wins, and the output is
 * then the identity; an empty segment gives the identity with status 0; a refused segment reads 2.  Points are decoded with flags 0, as
 * bn254_batch_g2_mul and bn254_batch_g2_sum decode them: on the curve, NO subgroup check.
 * Cost: a term kernel, one lane per term (decode, the 256-step ladder of bn254_batch_g2_mul, the Jacobian result to scratch — no inversion
 * per term), then one sum per segment in the collect's two layouts, split by BN254_OPT_COLLECT_WAVE_MIN_SHARES as in G1 (the split was
 * not swept for G2); one inversion per segment.
 * Measured on an MI355X (tools/dealing_throughput.py, profiles/dealing.jsonl; host forms under a host clock, staging on both sides, median
 * [min, max] of 7 alternating runs after 2 warm-up runs; against bn254_batch_g2_mul + bn254_batch_g2_sum): 65 536 terms in 4 096 segments
 * of 16 — the first length the wave layout takes — 8.59 ms [8.50, 8.92] against 8.00 [7.87, 18.0]: 0.6 ms SLOWER; 65 536 terms in one segment
 * 35.1 ms [34.95, 35.25] against 1 618 [1 566, 2 077], where g2_sum walks the segment in one lane; 171 terms in one segment 5.37 [5.33, 5.38]
 * against 9.69 [9.35, 10.55].  The _device form under events: 8.50, 35.04 and 5.33 ms.  Which call when: this one for long segments, for few
 * segments, or where the products are not wanted; the two old calls for many segments of about 16.  Unmeasured: other segment lengths, a
 * sweep of the lane/wave split.
 * DESIGN.md section 10m. */
int bn254_batch_g2_msm(bn254_ctx *ctx, const uint8_t *points /* m*128 */, const uint8_t *scalars /* m*32, big-endian */,
                       const uint64_t *seg_off /* n+1 */, size_t n, int reduce_scalar, uint8_t *out /* n*128 */, uint8_t *status /* n */);
int bn254_batch_g2_msm_device(bn254_ctx *ctx, const uint8_t *d_points, const uint8_t *d_scalars, const uint64_t *d_seg_off, size_t n,
                              int reduce_scalar, uint8_t *d_out, uint8_t *d_status, void *stream);

/* aggregate verify over shared pools (BASELINE config 3): tuple i names a message tuple_msg[i] and a
 * list of signers signer_idx[tuple_off[i] .. tuple_off[i+1]); status[i] = ECDSA::verify(msg, sum of the
 * listed signers' signatures on that message, sum of their public keys) — aggregation is plain point
 * addition (src/types.rs:126-132, :264-270) and only meaningful for one common message (src/lib.rs:34-38).
 * sig_pool[(m * n_signers + s) * 64]: signature of signer s on message m; pk_pool[s * 128].
 * An out-of-range signer index or message index (tuple_msg[i] >= n_msgs) gives status 2 (IndexOutOfBounds), as does
 * a decreasing tuple_off pair in the _device variant; an undecodable pool entry gives its decode status to every
 * tuple that uses it.  d_signer_idx must hold at least d_tuple_off[n] entries. */
int bn254_batch_aggregate_verify(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n_msgs+1 */, size_t n_msgs,
                                 const uint8_t *pk_pool /* n_signers*128 */, size_t n_signers, const uint8_t *sig_pool /* n_msgs*n_signers*64 */,
                                 const uint32_t *tuple_msg /* n */, const uint64_t *tuple_off /* n+1 */, const uint32_t *signer_idx, size_t n,
                                 uint32_t flags, uint8_t *status /* n */);
int bn254_batch_aggregate_verify_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t n_msgs, const uint8_t *d_pk_pool,
                                        size_t n_signers, const uint8_t *d_sig_pool, const uint32_t *d_tuple_msg, const uint64_t *d_tuple_off,
                                        const uint32_t *d_signer_idx, size_t n, uint32_t flags, uint8_t *d_status, void *stream);
/* REGISTERED POOLS — the aggregate counterpart of bn254_ctx_register_keys, for a caller whose pools are fixed (a validator set and the
 * messages it has signed) while tuples keep arriving: everything that depends on the pools alone — decoding, H(m) of every message, the
 * subset-sum tables of both pools (8 / 16 keys and 4 / 8 signatures per entry; ~8 ms per call for 1 024 x 1 024 pools) — is done ONCE.
 * expect_tuples = the batch size the tables are chosen for (the thresholds BN254_OPT_AGG_SUBSET_MIN_TUPLES / _AGG_WIDE_MIN_TUPLES are applied
 * to it; 0 = no tables).  bn254_batch_aggregate_verify_registered[_device] then takes only the tuples: same status bytes as
 * bn254_batch_aggregate_verify on the same pools (pool-entry decode statuses included; flags as given at registration).  The tables live in
 * the context until the next registration OR the next bn254_batch_aggregate_verify* call with raw pools (which reuses the same buffers):
 * after either, the registered call returns BN254_E_BAD_ARGUMENT until pools are registered again.  Reference: the sums are
 * `Add for PublicKey / Signature` (src/types.rs:126-132, :264-270), the check ECDSA::verify (src/ecdsa.rs:49-64). */
int bn254_ctx_register_pools(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n_msgs+1 */, size_t n_msgs, const uint8_t *pk_pool /* n_signers*128 */,
                             size_t n_signers, const uint8_t *sig_pool /* n_msgs*n_signers*64 */, uint32_t flags, size_t expect_tuples);
int bn254_ctx_register_pools_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t n_msgs, const uint8_t *d_pk_pool, size_t n_signers,
                                    const uint8_t *d_sig_pool, uint32_t flags, size_t expect_tuples, void *stream);
int bn254_batch_aggregate_verify_registered(bn254_ctx *ctx, const uint32_t *tuple_msg /* n */, const uint64_t *tuple_off /* n+1 */, const uint32_t *signer_idx,
                                            size_t n, uint8_t *status /* n */);
int bn254_batch_aggregate_verify_registered_device(bn254_ctx *ctx, const uint32_t *d_tuple_msg, const uint64_t *d_tuple_off, const uint32_t *d_signer_idx,
                                                   size_t n, uint8_t *d_status, void *stream);

/* Aggregate signatures over DISTINCT messages (the IRTF BLS draft's AggregateVerify, cited at src/lib.rs:26-31): the pairs j in
 * [agg_off[i], agg_off[i+1]) belong to aggregate i — message m_j = msgs[msg_off[j] .. msg_off[j+1]), key pk_j = pks[j*128] — whose
 * signature agg_sigs[i*64] is the sum of the signers' signatures (`Add for Signature`, src/types.rs:264-270).  status[i] is the first of:
 *   1. sigma_i's decode status, exactly as bn254_batch_verify decodes a signature (same flags);
 *   2. the decode status of the first pk_j in j order that fails (BN254_FLAG_G2_SUBGROUP_CHECK / _REJECT_IDENTITY act as in verify);
 *   3. the status of the first m_j that fails to hash: 1 (HashToPointError); in the _device form 5 for reversed or over-long offsets;
 *   4. 0 if pairing_batch([(H(m_j), pk_j)..., (sigma_i, -G2::one())]) == Gt::one(), else 9.
 * Consequences: k = 1 gives byte for byte the statuses of bn254_batch_verify on the same inputs; an EMPTY aggregate (k = 0) checks
 * e(sigma, -G2) == 1, i.e. it is 0 iff sigma is the identity and the identity is accepted.
 * Host form: agg_off[0] == 0, agg_off non-decreasing and agg_off[n] == m, msg_off non-decreasing, m, n < 2^32; anything else returns
 * BN254_E_BAD_ARGUMENT.  _device form: an aggregate whose range is reversed, runs past m or starts before an earlier offset (the ranges of
 * the accepted aggregates are disjoint) gets status 2 (IndexOutOfBounds) before anything else and no pairs — the convention of
 * bn254_batch_aggregate_verify_device for tuple_off; bn254_ctx_expect_msgs_len applies.
 * The check is exact (no random scalars).  Security: like the reference (src/lib.rs:34-38) it assumes a proof of possession of every key, and
 * NO distinct-message check is made — a caller who needs the draft's basic-scheme rule must enforce it.
 * Cost: one Miller loop per pair (two pairs of an aggregate share the squarings on a lane pair), one Miller loop of sigma and one final
 * exponentiation per aggregate.  One call reserves workspace for m pairs + m / 64 partial products + n aggregates (792 B each; no automatic
 * slicing): m is bounded by the device memory only (2^20 pairs in one aggregate take ~0.85 GB). */
int bn254_batch_aggregate_verify_distinct(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* m+1 */, const uint8_t *pks /* m*128 */,
                                          size_t m, const uint8_t *agg_sigs /* n*64 */, const uint64_t *agg_off /* n+1 */, size_t n, uint32_t flags,
                                          uint8_t *status /* n */);
int bn254_batch_aggregate_verify_distinct_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_pks, size_t m,
                                                 const uint8_t *d_agg_sigs, const uint64_t *d_agg_off, size_t n, uint32_t flags, uint8_t *d_status,
                                                 void *stream);

/* bn254_batch_aggregate_verify_distinct_keyed[_device]: as bn254_batch_aggregate_verify_distinct with key_idx[j] (uint32) in place of the
 * j-th public key: pk_j = the key registered at that index (bn254_ctx_register_keys).  Rule 2 takes, for the first failing key in j order,
 * 2 (IndexOutOfBounds) if key_idx[j] >= n_keys, else the key's registration status; with no keys registered every non-empty aggregate whose
 * sigma decodes gets 2.  An empty aggregate checks e(sigma, -G2) == 1 as before.  Same result bytes as
 * bn254_batch_aggregate_verify_distinct(flags | BN254_FLAG_G2_SUBGROUP_CHECK) on the expanded keys; for the keys,
 * BN254_FLAG_REJECT_IDENTITY is the one given at registration (the call's flags apply to sigma), as in bn254_batch_verify_keyed.  k = 1
 * everywhere gives byte for byte the statuses of bn254_batch_verify_keyed.  The host-form argument checks, the _device range rule (2 for a
 * reversed or overlapping agg_off), bn254_ctx_expect_msgs_len, BN254_E_MISALIGNED and the 2^32 limits are those of the unkeyed call.
 * Cost: every G2 argument is a line table (the keys' from registration, -G2's kept behind them), so the whole product of an aggregate is
 * ONE table-driven multi-Miller loop: its k + 1 pairs, sigma's included, take one or two per lane pair and no pair walks a twist point; no
 * separate Miller loop of sigma.  Contexts with pair lanes off and an empty key set expand the keys and take the unkeyed route.
 * Workspace: m pairs + partial products + n aggregates, nothing per key. */
int bn254_batch_aggregate_verify_distinct_keyed(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* m+1 */, const uint32_t *key_idx /* m */,
                                                size_t m, const uint8_t *agg_sigs /* n*64 */, const uint64_t *agg_off /* n+1 */, size_t n,
                                                uint32_t flags, uint8_t *status /* n */);
int bn254_batch_aggregate_verify_distinct_keyed_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint32_t *d_key_idx,
                                                       size_t m, const uint8_t *d_agg_sigs, const uint64_t *d_agg_off, size_t n, uint32_t flags,
                                                       uint8_t *d_status, void *stream);

/* bn254_batch_aggregate_verify_distinct_keyed_randomized[_device]: the same inputs and status bytes as bn254_batch_aggregate_verify_distinct_keyed,
 * with the pairing checks of many aggregates combined.  Rules 1-3 (sigma's decode; the first bad key: 2 out of range, else its registration
 * status; the first hash failure, or in the _device form a range error) are exact, and so are the host-form argument checks, the _device
 * range rule, bn254_ctx_expect_msgs_len, BN254_E_MISALIGNED and the 2^32 limits, which are the keyed call's.  A non-zero status is always the
 * exact one; a zero is wrong with probability <= 2^-128 per group (2^-64 with BN254_FLAG_RAND64) for a fresh secret seed32.
 *   r_i = rand_scalar(seed32, i) as in the other randomised calls (SHA-256(seed32 || le64(i)), 0 -> 1) with i = the aggregate's index in the
 *   call; BN254_FLAG_RAND64 and BN254_FLAG_RAND_GLV as documented there; the other flags apply to sigma, as in the keyed call.
 *   Groups: aggregate i belongs to group agg_off[i] / G, G = max(BN254_OPT_AGG_RAND_GROUP_PAIRS, n_keys) — consecutive whole aggregates;
 *   aggregates with a non-zero status from rules 1-3 take no part.  A group passes iff
 *       prod_key e(sum_{i in g} r_i sum_{j in i, key_idx[j] = key} H(m_j), pk_key) * e(sum_{i in g} r_i sigma_i, -G2) == 1
 *   — one table-driven multi-Miller loop over (distinct keys of the group + 1) pairs and one final exponentiation per group; messages that
 *   share a key within a group cost G1 additions, not Miller loops.  A group with ONE aggregate at the check takes r = 1: its check is the
 *   exact one with equal keys merged, and its status is that check's.  Every aggregate of a failed group of two or more is re-checked
 *   exactly on the device, with no host synchronisation (the _device form only enqueues).
 *   The exact keyed route, same bytes, when no keys are registered, pair lanes are off, or m < BN254_OPT_AGG_RAND_MIN_PAIRS.
 * Security: as bn254_batch_aggregate_verify_distinct — proof of possession of the registered keys is assumed, and the messages are not
 * checked for distinctness.  seed32 is host memory in both forms. */
int bn254_batch_aggregate_verify_distinct_keyed_randomized(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* m+1 */,
                                                           const uint32_t *key_idx /* m */, size_t m, const uint8_t *agg_sigs /* n*64 */,
                                                           const uint64_t *agg_off /* n+1 */, size_t n, uint32_t flags, const uint8_t *seed32,
                                                           uint8_t *status /* n */);
int bn254_batch_aggregate_verify_distinct_keyed_randomized_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                                  const uint32_t *d_key_idx, size_t m, const uint8_t *d_agg_sigs,
                                                                  const uint64_t *d_agg_off, size_t n, uint32_t flags,
                                                                  const uint8_t *seed32 /* host memory */, uint8_t *d_status, void *stream);

/* Same-message aggregates given as SIGNER BITMAPS over the registered keys — what a validator-set caller receives: one message m_i, one
 * already aggregated signature sigma_i (`Add for Signature`, src/types.rs:264-270) and a bitmap saying which of the keys registered with
 * bn254_ctx_register_keys signed.  Signer j of tuple i is bit j % 32 of signer_bits[i * bm_words + j / 32]; bm_words may be smaller than
 * ceil(n_keys / 32) (the keys beyond it are absent), larger, or 0 (signer_bits may then be NULL).  status[i] is the first of:
 *   1. sigma_i's decode status, exactly as bn254_batch_verify_keyed decodes a signature (the call's flags apply to sigma);
 *   2. for the LOWEST set bit j that is bad: 2 (IndexOutOfBounds) if j >= n_keys, else key j's non-zero registration status; with no keys
 *      registered any set bit gives 2;
 *   3. the hash status of m_i: 1 (HashToPointError); in the _device form 5 for reversed or over-long offsets (bn254_ctx_expect_msgs_len applies);
 *   4. 0 if e(H(m_i), sum_{j set} pk_j) * e(sigma_i, -G2::one()) == 1, else 9.
 * DEFINING IDENTITY: the status bytes are those of bn254_batch_aggregate_verify_distinct_keyed with the same flags on aggregates that repeat
 * m_i once per set bit, with key_idx = the set bits in ascending order — e(H(m), sum pk_j) = prod e(H(m), pk_j).  Consequences: an EMPTY
 * bitmap checks e(sigma, -G2) == 1; a registered identity key contributes nothing; a selection whose keys sum to the identity (a key and its
 * negation) behaves like the empty bitmap — the aggregate key is never "rejected as identity".  Security, as for the distinct-message calls:
 * a proof of possession of every registered key is assumed (src/lib.rs:34-38) — without one, rogue keys forge aggregates;
 * bn254_ctx_register_keys_pop registers a set with its proofs checked.
 * Argument checks, BN254_E_MISALIGNED (d_signer_bits is a 4-byte-aligned uint32 array) and the _device conventions are those of
 * bn254_batch_verify_keyed; BN254_OPT_MAX_CHUNK slices the tuples as there.
 * Cost: the aggregate key of a tuple is summed on the device from SUBSET TABLES of the registered set — the 256 subset sums of every 8
 * consecutive keys (5 152 B of device memory per registered key), so that a byte of a bitmap selects one table entry: n_keys / 8 additions
 * per tuple whatever the popcount, zero bytes skipped — then ONE verify per tuple (the routing table serves small batches with the small-batch
 * kernels).  The tables and a bad-key bit vector are built lazily, on the call's stream, by the first bitmap call after a registration
 * (bn254_ctx_register_keys invalidates them; its own cost and behaviour are unchanged); the context's one-call-in-flight rule orders every
 * later call behind the build.  Key sets above BN254_OPT_BITMAP_TABLE_MAX_KEYS are summed key by key (popcount additions); same status bytes.
 * Which call when: this one whenever the tuples share their message — it costs one verify + n_keys / 8 additions per tuple, where
 * bn254_batch_aggregate_verify_distinct_keyed with the message repeated costs one table-driven Miller pair per signer.  Measured on an MI355X,
 * 65 536 tuples over 256 keys: 10.5 ms against 407 ms with two thirds of the bits set, 11.0 against 13.2 ms with ONE bit set per tuple — no
 * popcount at which the other call wins was found. */
int bn254_batch_verify_keyed_bitmap(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */, const uint8_t *sigs /* n*64 */,
                                    const uint32_t *signer_bits /* n*bm_words */, size_t bm_words, size_t n, uint32_t flags, uint8_t *status /* n */);
int bn254_batch_verify_keyed_bitmap_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_sigs,
                                           const uint32_t *d_signer_bits, size_t bm_words, size_t n, uint32_t flags, uint8_t *d_status, void *stream);

/* bn254_batch_verify_keyed_bitmap_randomized[_device]: the same inputs and status bytes as bn254_batch_verify_keyed_bitmap with the same flags,
 * with the pairing checks of many tuples combined.  Rules 1-3 (sigma's decode, the lowest bad bit, the hash status) are exact, and so are the
 * argument checks, BN254_E_MISALIGNED, the _device conventions and the BN254_OPT_MAX_CHUNK slicing, which are the bitmap call's.  A non-zero
 * status is always the exact one; a zero is wrong with probability <= 2^-128 per group (2^-64 with BN254_FLAG_RAND64) for a fresh secret seed32.
 *   r_i = rand_scalar(seed32, i) as in the other randomised calls (SHA-256(seed32 || le64(i)), 0 -> 1) with i = the tuple's index in the
 *   caller's arrays, also under slicing; BN254_FLAG_RAND64 and BN254_FLAG_RAND_GLV as documented there; the other flags apply to sigma.
 *   Groups: tuple i of a slice belongs to group (i - slice_lo) / G, G = BN254_OPT_BITMAP_RAND_GROUP_TUPLES; tuples with a non-zero status from
 *   rules 1-3 take no part.  Every aggregate key is a sum over the registered set, so the combined check regroups by key: a group passes iff
 *       prod_j e(T_j, pk_j) * e(S, -G2) == 1,   T_j = sum_{i in g, bit j of tuple i} r_i H(m_i),   S = sum_{i in g} r_i sigma_i
 *   over the keys j with a contributor (registered identity keys take no part; a T_j that comes out as the identity contributes 1) — at most
 *   n_keys + 1 table-driven Miller pairs and ONE final exponentiation per group, every G2 argument a registered line table.  Per tuple there
 *   remain the hash, two scalar ladders and one G1 addition per non-zero bitmap BYTE (the byte buckets of a window are folded into its eight
 *   key sums once per group), whatever the popcount.  A group with ONE tuple at the check takes r = 1 and its verdict is final.  Every tuple
 *   of a failed group of two or more is verified exactly on the device (aggregate key by the bitmap call's summation, then a verify), with
 *   no host synchronisation (the _device form only enqueues).
 *   The exact bitmap call, same bytes, when no keys are registered, pair lanes are off, n < BN254_OPT_BITMAP_RAND_MIN_TUPLES, more keys are
 *   registered than BN254_OPT_BITMAP_RAND_MAX_KEYS, or the call (a
 *   slice of it) is so large that its buckets, sort elements or workspace entries would not be numbered in 32 bits.
 * Security: as bn254_batch_verify_keyed_bitmap — a proof of possession of every registered key is assumed.  seed32 is host memory in both forms.
 * Which call when (measured on an MI355X, every tuple valid, two thirds of the keys signing, 128-bit weights): over
 * 256 keys this call from 81 920 tuples on — 13.2 ms against the exact call's 16.9 there, 17.8 against 20.7 at 131 072, 104 against 165 ms at
 * 2^20 (1.58 x; 1.79 x with BN254_FLAG_RAND64) — and the exact call below: at 65 536 tuples it takes 11.1 ms against 10.6, at 16 384 6.7
 * against 4.9.  Over 1 024 keys the exact call at every size measured (65 536 tuples: 22.8 ms against 12.5): the G1 side costs one addition
 * per bitmap byte and tuple.  The defaults follow that: below BN254_OPT_BITMAP_RAND_MIN_TUPLES (81 920) tuples or above
 * BN254_OPT_BITMAP_RAND_MAX_KEYS (256) keys this call IS the exact call.  Key sets between 256 and 1 024 keys were not measured.  Where many
 * groups are expected to fail, the exact call: a failed group pays the exact price on top. */
int bn254_batch_verify_keyed_bitmap_randomized(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */, const uint8_t *sigs /* n*64 */,
                                               const uint32_t *signer_bits /* n*bm_words */, size_t bm_words, size_t n, uint32_t flags,
                                               const uint8_t *seed32, uint8_t *status /* n */);
int bn254_batch_verify_keyed_bitmap_randomized_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_sigs,
                                                      const uint32_t *d_signer_bits, size_t bm_words, size_t n, uint32_t flags,
                                                      const uint8_t *seed32 /* host memory */, uint8_t *d_status, void *stream);

/* WHAT A BITMAP CALL KNOWS BESIDES A STATUS BYTE — for the party that hands a bitmap aggregate on to a verifier that holds no validator set (a
 * contract, another chain): the aggregate public key, H(m) and the voting weight behind the bitmap.  Bitmaps are read as in
 * bn254_batch_verify_keyed_bitmap (bm_words smaller or larger than needed, or 0 with a NULL bitmap); the argument checks, the _device
 * conventions (device pointers, only enqueues, one call in flight per context) and the BN254_OPT_MAX_CHUNK slicing are that call's.
 *
 * A. bn254_batch_aggregate_keys_bitmap[_device]: status[i] is RULE 2 of the bitmap verify and nothing else — for the lowest bad set bit, 2 if
 *    it is at or above n_keys, else that key's registration status; with no keys registered any set bit gives 2.  Where status[i] == 0,
 *    agg_keys[i] is the uncompressed sum of the set keys — 128 zero bytes when the sum is the identity (an empty row, only identity keys, a
 *    key and its negation; the status stays 0) — and 128 zero bytes where status[i] != 0.  DEFINING IDENTITY: for a tuple of status 0 the
 *    bytes are those of bn254_batch_g2_sum over one segment holding the registered encodings of the set keys in ascending order.  The same
 *    bytes on every route of the sum (subset tables or key by key, lane pairs or one lane).  flags must be 0 (BN254_E_BAD_ARGUMENT);
 *    d_signer_bits and d_agg_keys are 4-byte aligned (BN254_E_MISALIGNED); n == 0 returns 0.  Cost: the bitmap verify's sum (n_keys / 8
 *    table additions and one inversion per tuple) and one encode kernel.
 *
 * B. bn254_batch_verify_keyed_bitmap_export[_device]: the status bytes are byte for byte those of bn254_batch_verify_keyed_bitmap with the
 *    same arguments and flags (BN254_FLAG_REJECT_IDENTITY and BN254_FLAG_G1_COMPRESSED included).  A tuple whose status is 0 or 9 has
 *    passed rules 1-3: hashes[i] is the 64 bytes bn254_batch_hash_to_g1 gives for m_i and agg_keys[i] the 128 bytes call A gives for row i.
 *    For every other tuple both outputs are zero bytes.  Either output pointer may be NULL; with both NULL the call is the verify.  The
 *    output pointers of the _device form are 4-byte aligned.  Profiling intervals as the bitmap verify's (the emit counts in ms[1]).
 *    H(m), the key and the signature are what the reference's precompile formatters take (src/utils.rs:197-239).
 *
 * C. bn254_ctx_set_key_weights gives registered key j the voting weight weights[j] (host memory; NULL forgets the weights).  Host-synchronous,
 *    quiesces like a registration.  BN254_E_BAD_ARGUMENT if n_keys differs from the registered count or the weights total 2^64 or more (so no
 *    subset sum wraps); a refused call leaves no weights set.  EVERY registration call forgets the weights: a new set is a new committee.
 *    bn254_batch_bitmap_weights[_device] (BN254_E_BAD_ARGUMENT while no weights are set): status[i] is rule 2 as in A, weight[i] the sum of
 *    the set keys' weights where the status is 0, else 0.  A registered IDENTITY key counts its weight — it is a member with status 0; a
 *    set that must not hold one registers with BN254_FLAG_REJECT_IDENTITY.  The calls read bitmaps only: the used_bits rows of the collect,
 *    merge and threshold calls go straight in.  d_weight is 8-byte aligned.  The caller compares the weight with its quorum.  Cost: one
 *    lookup per bitmap byte in tables of u64 subset sums (2 KB of device memory per 8 keys), one path at every size; the call takes no
 *    workspace and is not sliced.
 * Measured on an MI355X (profiles/bitmap_out.jsonl; median of 7 alternating runs, whole host-pointer calls, two thirds of 256 keys signing;
 * DESIGN.md section 10q has the spreads): at 65 536 tuples the export call 11.9 ms against 320 ms for the route that existed (bitmap verify +
 * bn254_batch_hash_to_g1 + host gather of 22 KB per tuple + bn254_batch_g2_sum) and 10.9 for the plain verify; at 256 tuples 1.59 against 7.44
 * and 1.58; 256 tuples over 4 096 keys 6.36 against 96.3 and 6.40.  Under events the _device export equals the _device verify within its
 * spread (10.51 ms both).  Keys alone: 1.07 against 315 ms, 0.40 against 5.7, 5.2 against 90.  Weights: 0.21 ms against 17.2 for a numpy bit
 * walk at 65 536 tuples, but 0.049 against 0.034 at 256 — a host caller with a few hundred bitmaps may walk them itself; the _device form
 * takes 0.026 / 0.015 ms.  Which call when: the export call whenever H(m) or the key is wanted beside the verdict; call A for keys without a
 * signature.  Unmeasured: key sets between 256 and 4 096, compressed sigmas on the export, failing tuples at scale. */
int bn254_batch_aggregate_keys_bitmap(bn254_ctx *ctx, const uint32_t *signer_bits /* n*bm_words */, size_t bm_words, size_t n,
                                      uint32_t flags /* must be 0 */, uint8_t *agg_keys /* n*128 */, uint8_t *status /* n */);
int bn254_batch_aggregate_keys_bitmap_device(bn254_ctx *ctx, const uint32_t *d_signer_bits, size_t bm_words, size_t n, uint32_t flags,
                                             uint8_t *d_agg_keys, uint8_t *d_status, void *stream);
int bn254_batch_verify_keyed_bitmap_export(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */, const uint8_t *sigs /* n*64 */,
                                           const uint32_t *signer_bits /* n*bm_words */, size_t bm_words, size_t n, uint32_t flags,
                                           uint8_t *status /* n */, uint8_t *hashes /* n*64, or NULL */, uint8_t *agg_keys /* n*128, or NULL */);
int bn254_batch_verify_keyed_bitmap_export_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_sigs,
                                                  const uint32_t *d_signer_bits, size_t bm_words, size_t n, uint32_t flags, uint8_t *d_status,
                                                  uint8_t *d_hashes, uint8_t *d_agg_keys, void *stream);
int bn254_ctx_set_key_weights(bn254_ctx *ctx, const uint64_t *weights /* n_keys, host; NULL: forget */, size_t n_keys);
int bn254_batch_bitmap_weights(bn254_ctx *ctx, const uint32_t *signer_bits /* n*bm_words */, size_t bm_words, size_t n, uint64_t *weight /* n */,
                               uint8_t *status /* n */);
int bn254_batch_bitmap_weights_device(bn254_ctx *ctx, const uint32_t *d_signer_bits, size_t bm_words, size_t n,
                                      uint64_t *d_weight /* 8-byte aligned */, uint8_t *d_status, void *stream);

/* BUILDING a signer-bitmap aggregate — the producer half of bn254_batch_verify_keyed_bitmap: per message the node holds individual signatures
 * ("shares"), each said to be by one registered key, and needs every share checked against its key (one bad share poisons the sum, and the
 * sum cannot say which), the sum of those that passed, and the bitmap of who they were.  Tuple i is the message msgs[msg_off[i] ..
 * msg_off[i+1]) and the shares s in [share_off[i], share_off[i+1]); share s is the signature shares[64 s] said to be by registered key
 * share_key[s].  share_status[s] is the first of:
 *   1. the share's decode status, exactly as bn254_batch_verify_keyed decodes a signature (the call's flags apply);
 *   2. 2 (IndexOutOfBounds) if share_key[s] >= n_keys, else the key's non-zero registration status; with no keys registered every share
 *      that decodes gets 2;
 *   3. the hash status of the tuple's message: 1 (HashToPointError); in the _device form 5 for reversed or over-long message offsets
 *      (bn254_ctx_expect_msgs_len applies);
 *   4. 0 if e(H(m_i), pk_key) * e(share, -G2::one()) == 1, else 9.
 * DEFINING IDENTITY 1: share_status is byte for byte what bn254_batch_verify_keyed returns, with the same flags, for n_shares items whose
 * message is their tuple's message repeated.
 * tuple_status[i] is 0, the hash status of m_i (1 or 5), or — in the _device form, and ahead of the hash status — 2 for a share range that
 * is reversed, runs past n_shares, or starts before an earlier offset (the range rule of bn254_batch_aggregate_verify_distinct_device).
 * Such a tuple gets an empty bitmap, the identity as its aggregate and no shares; share_status is first filled with 2, so a share that
 * belongs to no accepted tuple reads 2.
 * Outputs of an accepted tuple:
 *   - signer_bits row i, in the bitmap call's numbering (signer j = bit j % 32 of word i * bm_words + j / 32): bit j is set iff some share of
 *     the tuple with share_key == j has status 0; words past the key set are zero;
 *   - agg_sigs[i]: the sum of ONE status-0 share per set bit, uncompressed, the identity as 64 zero bytes;
 *   - n_signers[i] (the array may be NULL): the popcount of row i.
 * A key that sent several valid shares counts once.  G1 has prime order, so the valid signature of (m, pk) is unique: the duplicates are the
 * same point, the result does not depend on which of them is taken, and the sum may be formed in parallel in any order — the bytes are the
 * same.  Two different indices that hold the same key both count, as the bitmap verify sums both.
 * Argument checks: bm_words >= ceil(n_keys / 32) — a bitmap that cannot hold a registered key cannot describe the result — and bm_words <=
 * 0xFFFFFFFF, else BN254_E_BAD_ARGUMENT; n and n_shares < 2^32; host form: share_off[0] == 0, non-decreasing, share_off[n] == n_shares.
 * BN254_E_MISALIGNED as in the bitmap call: shares, share_key, agg_sigs, signer_bits and n_signers 4-byte aligned, the offsets 8-byte
 * aligned.  n == 0 returns 0.  BN254_OPT_MAX_CHUNK slices the SHARES (and the tuples' hashing) freely; the outputs are the same.
 * DEFINING IDENTITY 2 (closed loop, flags = 0): bn254_batch_verify_keyed_bitmap(msgs, agg_sigs, signer_bits, bm_words) on the call's own
 * outputs returns 0 for every tuple with tuple_status == 0 — the tuple with no valid share (empty bitmap, identity signature) and a key and
 * its negation both signing (two bits set, the aggregate is the identity) included.
 * Cost: ONE hash-to-G1 per tuple (not per share), one keyed verify per share (the routing table and the line tables of
 * bn254_batch_verify_keyed, unchanged), and one G1 addition per counted share in a select-and-sum launched once behind the last slice: a
 * tuple of fewer than BN254_OPT_COLLECT_WAVE_MIN_SHARES shares is walked by one lane, a longer one by the 64 lanes of a wave (bits claimed
 * with atomic ORs on the zeroed row, 64 partial sums folded by six levels of additions in LDS).  The _device form only enqueues: no host
 * synchronisation, the range rule included.  Measured on an MI355X (tools/collect_throughput.py, profiles/collect_throughput.jsonl; 256 keys,
 * every share valid; per-stage times from bn254_ctx_last_kernel_ms): 256 tuples x 171 shares — front end 0.19 ms, select-and-sum 0.24, Miller
 * loop 4.03, final exponentiation 3.61, against the keyed verify's 0.03 + 0.32 (hash) + 4.05 + 3.60 on the 43 776 repeated messages;
 * 4 096 x 11 — 0.32, 0.18, 3.99, 3.58 against 0.01 + 0.33 + 4.01 + 3.59; one tuple of 4 096 shares — 0.22, 0.27 (one wave), 1.06, 1.14:
 * the sum is an eighth of its verify (one lane: 4.6 ms).  So the device work exceeds the keyed verify's by about 0.1 ms: hashing once saves
 * less than the spread and the sum cost.  What the call spares a caller of bn254_batch_verify_keyed_device is what followed that verify: the
 * copy of the statuses to the host, the filter there, and bn254_batch_g1_sum, whose host-pointer form stages every share again and walks each
 * segment in one lane.  Whole-call intervals of both routes, as far as they were measured: DESIGN.md section 10e.
 * Which call when: this one for calls of few shares, or of few shares per registered key; bn254_batch_collect_keyed_bitmap_randomized below where
 * the keys have many shares each across the tuples of the call.
 * Compressed shares: BN254_FLAG_G1_COMPRESSED (33 bytes per share, no alignment).  Out of scope: the multi-GPU layer. */
int bn254_batch_collect_keyed_bitmap(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */,
                                     const uint8_t *shares /* n_shares*64 */, const uint32_t *share_key /* n_shares */,
                                     const uint64_t *share_off /* n+1 */, size_t n_shares, size_t n, size_t bm_words, uint32_t flags,
                                     uint8_t *share_status /* n_shares */, uint8_t *tuple_status /* n */, uint8_t *agg_sigs /* n*64 */,
                                     uint32_t *signer_bits /* n*bm_words */, uint32_t *n_signers /* n, or NULL */);
int bn254_batch_collect_keyed_bitmap_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_shares,
                                            const uint32_t *d_share_key, const uint64_t *d_share_off, size_t n_shares, size_t n, size_t bm_words,
                                            uint32_t flags, uint8_t *d_share_status, uint8_t *d_tuple_status, uint8_t *d_agg_sigs,
                                            uint32_t *d_signer_bits, uint32_t *d_n_signers, void *stream);

/* bn254_batch_collect_keyed_bitmap_randomized[_device]: the same inputs and, byte for byte, the same five outputs as
 * bn254_batch_collect_keyed_bitmap[_device] with the same flags — share_status, tuple_status, agg_sigs, signer_bits and n_signers — with the
 * pairing checks of the shares combined.  Rules 1-3 of share_status (decode, key index and registration status, the tuple's hash status) are
 * exact; a non-zero share_status is always the exact one; a zero is wrong with probability <= 2^-128 per group (2^-64 with BN254_FLAG_RAND64)
 * for a fresh secret seed32.  Defining identities 1 and 2 carry over.  The argument checks, BN254_E_MISALIGNED, the range rule, the fill of
 * share_status with 2 and the _device conventions are the exact call's: no host synchronisation, every buffer reserved before the first kernel.
 *   r_s = rand_scalar(seed32, s) as in the other randomised calls (the first 16 — 8 with BN254_FLAG_RAND64 — bytes of SHA-256(seed32 ||
 *   le64(s)), little-endian, 0 -> 1) with s = the share's index in the caller's arrays, also under slicing.  BN254_FLAG_RAND64 and
 *   BN254_FLAG_RAND_GLV mean what they mean in bn254_batch_verify_keyed_randomized; the other flags apply to the shares' decode.
 *   Groups: the shares of a tuple share H(m), not the key — but across the TUPLES of a call every registered key has many shares.  Within a
 *   slice of the shares, those that pass rules 1-3 are grouped by key in runs of 64, exactly as bn254_batch_verify_keyed_randomized groups its
 *   items, and a group passes iff
 *       e(sum_s r_s H(m_t(s)), pk) * e(sum_s r_s share_s, -G2) == 1      (t(s) = the tuple of share s)
 *   — two table-driven Miller loops and one final exponentiation per 64 shares, and per share two scalar ladders.  The shares of a passing
 *   group get 0; every share of a failing group is verified exactly on the device.  Select-and-sum runs once behind the last slice, unchanged.
 *   A slice is as long as BN254_OPT_MAX_CHUNK says, or as its slots TOGETHER WITH its group entries (len / 64 + min(n_keys, len) + 1 of them,
 *   behind the slots) fit the workspace.
 *   The exact call, same bytes, when no keys are registered, n_shares < BN254_OPT_COLLECT_RAND_MIN_SHARES, n_shares / n_keys <
 *   BN254_OPT_COLLECT_RAND_MIN_PER_KEY (groups are per key: a call whose keys have one or two shares each buys padding, not speed), or no
 *   slice with its groups fits.  Both thresholds are the most the host can know without looking at share_key.
 * The seed must be secret and fresh: who knows r can forge a pair of shares of one key whose errors cancel in the group's sum
 * (share_1 + r_2 D, share_2 - r_1 D pass together), and both would then be summed into aggregates that do not verify.
 * seed32 is host memory in both forms.  Profiling: bn254_ctx_last_kernel_ms keeps the exact call's four intervals; ms[2] and ms[3] mean
 * "grouping + scalar ladders" and "group checks + exact re-checks" here.
 * Which call when (measured on an MI355X, every share valid, tuples of 171 shares, whole-call medians on a caller's stream; DESIGN.md section
 * 10f): over 256 keys this call from 65 664 shares on — 9.3 ms against the exact call's 13.4 there, 13.0 against 24.0 at 175 104, 18.3 against
 * 42.9 at 350 208 (2.3 x; 13.3 ms, 3.2 x, with BN254_FLAG_RAND64) — and the exact call below: at 43 776 shares it takes 8.7 ms against 8.2
 * (64-bit weights: 7.7), at 4 104 shares 7.4 against 2.6.  The group checks are ONE pass of the lane-pair keyed kernels over a few hundred to
 * a few thousand groups, 4.7 ms whatever their number, which is what a small call cannot win back.  Over 4 096 keys: 175 104 shares (42 per
 * key) 15.5 ms against 24.2, but 43 776 shares (10 per key) 13.5 against 8.3 — every key's run is padded to whole groups of 64, and the
 * ladders are paid per slot.  The defaults follow that: below BN254_OPT_COLLECT_RAND_MIN_SHARES (65 664) shares, or below
 * BN254_OPT_COLLECT_RAND_MIN_PER_KEY (42) shares per registered key, this call IS the exact call.  Not measured: between 45 056 and 65 664
 * shares, and between 10 and 42 shares per key.  Where many shares are expected to be wrong, the exact call: 1 % wrong shares spread over the
 * tuples fail 44 % of the groups of 256 x 171 and the call takes 13.4 ms against 8.0. */
int bn254_batch_collect_keyed_bitmap_randomized(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */,
                                                const uint8_t *shares /* n_shares*64 */, const uint32_t *share_key /* n_shares */,
                                                const uint64_t *share_off /* n+1 */, size_t n_shares, size_t n, size_t bm_words, uint32_t flags,
                                                const uint8_t *seed32, uint8_t *share_status /* n_shares */, uint8_t *tuple_status /* n */,
                                                uint8_t *agg_sigs /* n*64 */, uint32_t *signer_bits /* n*bm_words */,
                                                uint32_t *n_signers /* n, or NULL */);
int bn254_batch_collect_keyed_bitmap_randomized_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_shares,
                                                       const uint32_t *d_share_key, const uint64_t *d_share_off, size_t n_shares, size_t n,
                                                       size_t bm_words, uint32_t flags, const uint8_t *seed32 /* host memory */,
                                                       uint8_t *d_share_status, uint8_t *d_tuple_status, uint8_t *d_agg_sigs,
                                                       uint32_t *d_signer_bits, uint32_t *d_n_signers, void *stream);

/* bn254_batch_collect_keyed_bitmap_optimistic[_device]: the exact collect's arguments and five outputs, with ONE verify per tuple.  The
 * shares of a tuple share the message: if every share is good, their sum is the aggregate of the tuple's bitmap, and
 *     e(H(m_i), sum_{j in row} pk_j) * e(sum_j share_j, -G2) == 1
 * proves it.  Only a tuple whose sum fails needs its shares checked one by one.  No randomness, no seed.  The argument checks,
 * BN254_E_MISALIGNED, the range rule, the fill of share_status with 2 and the _device conventions are those of
 * bn254_batch_collect_keyed_bitmap[_device]: no host synchronisation, every buffer reserved before the first kernel; BN254_OPT_MAX_CHUNK
 * slices the shares (of the exact fallback) and the tuples (of the hash and of the tuple check) as it does there.
 *   1. PRE-CHECK.  Every share of an accepted tuple gets its status from rules 1-3 of the exact collect, with the call's flags: the decode
 *      status; 2 for share_key >= n_keys, or the key's non-zero registration status; the tuple's hash status.  No pairing is computed.  A
 *      share with status 0 here is a CANDIDATE.
 *   2. ELIGIBILITY, decided per tuple on the device: at least BN254_OPT_COLLECT_OPT_MIN_TUPLE_SHARES candidates, and no two candidates that
 *      name the same key index.  Honest traffic has no duplicates; a tuple with one goes the exact way, so "which duplicate is taken" never
 *      arises on this route and the outcome does not depend on the order in which racing lanes claim bits.
 *   3. PROVISIONAL RESULT of an eligible tuple: the bitmap row is its candidates' keys, the aggregate their sum, the count the popcount.  A
 *      tuple with no candidate is final as it stands: empty row, identity, 0.
 *   4. TUPLE CHECK.  Each eligible tuple gets one verify, e(H(m_i), sum_{j in row} pk_j) * e(agg_i, -G2) == 1: H(m_i) was hashed once, the
 *      aggregate key comes from the bitmap call's subset tables, and the decode flags are 0 for this step — an identity aggregate is
 *      legitimate (a key and its negation both signing).  The kernels are those of bn254_batch_verify_keyed_bitmap, so a small n is served
 *      by the small-batch kernels of the routing table.
 *   5. PASS.  The provisional outputs of a passing tuple are final, and its candidates keep status 0.
 *   6. FALLBACK.  The tuples that fail the check, that have a duplicate, or that have fewer candidates than the per-tuple minimum go into a
 *      device-side queue with their candidates.  The queued candidates are verified exactly by the keyed kernels (rule 4 of the exact
 *      collect: 0 or 9) — the Miller loop and the final exponentiation run over queued shares only, though every share of a slice is decoded
 *      and spread again; the tuples' rows are zeroed and select-and-sum runs again for these tuples only, with the exact call's rule.  Their
 *      outputs are byte for byte the exact call's.
 *   7. WHOLE-CALL ROUTING.  The call IS the exact call (same bytes) when no keys are registered or n_shares < BN254_OPT_COLLECT_OPT_MIN_SHARES.
 * IDENTITY 2 OF THE EXACT COLLECT HOLDS UNCONDITIONALLY: bn254_batch_verify_keyed_bitmap with flags 0 on the call's own outputs returns 0 for
 * every tuple with tuple_status == 0 — a passing tuple has just been verified so, a fallback tuple is the exact call's.
 * EQUALITY WITH THE EXACT CALL: all five outputs equal bn254_batch_collect_keyed_bitmap's whenever no passing tuple contains a candidate that
 * the exact call would have given 9.
 * THE ONE DEVIATION: candidates whose errors cancel — share_a + D and share_b - D from two cooperating signers — read 0 and are counted here;
 * the exact call gives both 9.  What comes out is still the valid aggregate share_a + share_b for bits a and b.  A status 0 inside a passing
 * tuple therefore means "counted in a sum that verifies", not "individually valid"; a caller who needs per-share verdicts, for slashing say,
 * uses the exact call.  Defining identity 1 of the exact collect holds only up to this deviation.
 * Proof of possession of the registered keys is assumed, as everywhere in this family.
 * Cost: with every share valid the Miller loop and the final exponentiation run over n tuples instead of n_shares shares; per share remain
 * the decode of the pre-check, one G1 addition, and the decode and spread of the fallback's front end, which runs whether or not anything
 * is queued (the host never learns).  With every tuple failing the call costs the exact call plus one n-item verify pass.
 * Which call when (measured on an MI355X, tools/collect_throughput.py --optimistic, whole-call medians on a caller's stream, inputs
 * resident, 256 keys).  Every share valid: 256 tuples x 171 shares 1.87 ms against the exact call's 8.24 and the
 * randomised call's 8.71; 1 024 x 171 2.54 against 24.4 and 12.6; 2 048 x 171 2.85 against 44.6 and 18.4 (15.7 x, 6.5 x); 4 096 x 11 3.25
 * against 8.29; 24 x 171 1.85 against 2.56; 9 x 171 (1 539 shares) 1.86 against 2.09 — but 6 x 171 ties (1.83) and 3 x 171 loses (1.84
 * against 1.38): the call is one verify pass of n items plus 0.9 ms whatever the shares.  Over 4 096 keys 256 x 171 takes 6.71 ms against
 * 8.15: the aggregate keys cost 5.2 ms there (the bitmap verify's sum, unchanged).  ANY tuple that goes the exact way costs the call one pass
 * of the queue's lane-pair kernels, 4.9 ms whether it queues 11 shares or 5 000: one failing tuple takes 256 x 171 to 6.73 ms (still below
 * the exact call), 2 048 x 171 to 7.78 (against 44.6), but 24 x 171 to 6.70 against the exact call's 2.56.  1 % wrong shares spread over
 * tuples of 171 fail every tuple: 10.0 ms against 8.07 at 256 x 171, 47.9 against 44.3 at 2 048 x 171 — the exact call plus the optimistic
 * pass.  Tuples of ONE or TWO shares lose (4 096 x 1: 3.33 against 2.51; 4 096 x 2: 3.31 against 2.54; 16 384 x 1: 5.47 against 4.60 — a
 * tuple check per share or two is no saving), tuples of four win (4 096 x 4: 3.31 against 4.66); three were not measured.  A tuple that
 * lists a key twice sends itself the exact way (1 x 4 096 over 256 keys: 6.89 against 2.62).  So: this call where tuples have four or more
 * shares, almost all valid, and the call has 1 539 shares or more (BN254_OPT_COLLECT_OPT_MIN_SHARES); the exact call for small calls, for
 * per-share verdicts, where more than the odd tuple is expected to hold a wrong share and the call is one the exact route serves in under
 * 5 ms, and for calls made of one- or two-share tuples (the host-side thresholds cannot see the shape).  Not measured: between 1 026 and
 * 1 539 shares, tuples of 3 and of 12 .. 170 shares, key sets between 256 and 4 096 keys, wrong shares over 4 096 keys beyond 256 x 171.
 * Profiling: ms[0] = front end (hash, range rule, pre-check) and provisional sum, ms[1] = aggregate keys, ms[2] = the tuples' Miller loop and
 * final exponentiation, ms[3] = exact fallback and re-sum.
 * Compressed shares: BN254_FLAG_G1_COMPRESSED.  Out of scope: a randomised fallback, the multi-GPU layer. */
int bn254_batch_collect_keyed_bitmap_optimistic(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */,
                                                const uint8_t *shares /* n_shares*64 */, const uint32_t *share_key /* n_shares */,
                                                const uint64_t *share_off /* n+1 */, size_t n_shares, size_t n, size_t bm_words, uint32_t flags,
                                                uint8_t *share_status /* n_shares */, uint8_t *tuple_status /* n */, uint8_t *agg_sigs /* n*64 */,
                                                uint32_t *signer_bits /* n*bm_words */, uint32_t *n_signers /* n, or NULL */);
int bn254_batch_collect_keyed_bitmap_optimistic_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_shares,
                                                       const uint32_t *d_share_key, const uint64_t *d_share_off, size_t n_shares, size_t n,
                                                       size_t bm_words, uint32_t flags, uint8_t *d_share_status, uint8_t *d_tuple_status,
                                                       uint8_t *d_agg_sigs, uint32_t *d_signer_bits, uint32_t *d_n_signers, void *stream);

/* MERGING partial signer-bitmap aggregates — the inner node of an aggregation tree.  A committee node receives, per message, a handful of
 * PARTIAL aggregates from its children (a bitmap and one summed signature each) and has to pass one aggregate upward: every partial verified
 * against its bitmap, the valid ones that do not overlap added, and the union bitmap written — on the device, with no host synchronisation,
 * the outputs going straight into bn254_batch_verify_keyed_bitmap.  Tuple i is the message msgs[msg_off[i] .. msg_off[i+1]) and the partials
 * p in [part_off[i], part_off[i+1]); partial p is the signature parts[64 p] with bitmap row p of part_bits (bm_words words, in the bitmap
 * verify's numbering: signer j = bit j % 32 of word p * bm_words + j / 32).
 * part_status[p], DEFINING IDENTITY 1: byte for byte what bn254_batch_verify_keyed_bitmap returns, with the same flags, for n_parts items whose
 * message is their tuple's message repeated — rules 1-4 there: sigma's decode status, the lowest bad bit (2 if it is >= n_keys, else the key's
 * registration status; with no keys registered any set bit gives 2), the hash status (1, or 5 in the _device form), then 0 or 9.  The
 * message is hashed once per tuple, not once per partial.  An empty row is verified as the bitmap call verifies it (e(sigma, -G2) == 1: only
 * the identity passes).  No new status code.
 * tuple_status[i] and the RANGE RULE are the exact collect's: 0, the hash status of m_i, or — in the _device form, and ahead of it — 2 for a
 * range that is reversed, runs past n_parts, or starts before an earlier offset.  part_status is filled with 2 first: a partial of no accepted
 * tuple reads 2, and its part_taken 0.  A refused tuple gets an empty row, the identity as its aggregate and count 0.
 * SELECT, part_taken[p] (1 or 0): within a tuple, IN THE CALLER'S ORDER, partial p is taken iff part_status[p] == 0 and its row is disjoint from
 * the union of the rows taken earlier in that tuple (first fit).  A partial that overlaps only partials that were themselves refused or not
 * taken is taken.  A status-0 partial with an empty row is taken and adds nothing: its signature is the identity.  A caller who wants the
 * largest cover sorts a tuple's partials by descending popcount.  First fit is well defined here because the valid aggregate of (m, set of
 * keys) is unique — G1 has prime order —, so the outputs depend only on WHICH rows are taken, never on which of two equal partials was, and the
 * sum may be formed in parallel in any order: the bytes are the same.
 * Outputs of an accepted tuple:
 *   - signer_bits row i: the OR of the taken rows;
 *   - agg_sigs[i]: the sum of the taken signatures, uncompressed, the identity as 64 zero bytes;
 *   - n_signers[i] (the array may be NULL): the popcount of row i.
 * DEFINING IDENTITY 2 (closed loop, flags = 0): bn254_batch_verify_keyed_bitmap(msgs, agg_sigs, signer_bits, bm_words) on the call's own
 * outputs returns 0 for every tuple with tuple_status == 0.
 * DEFINING IDENTITY 3 (the collect inside it): with bm_words >= ceil(n_keys / 32) and every partial's row holding exactly one bit, bit k_p,
 * part_status, tuple_status, agg_sigs, signer_bits and n_signers equal bn254_batch_collect_keyed_bitmap's with share_key = k_p, and
 * part_taken[p] is 1 exactly for the first status-0 share of its key in its tuple.
 * Argument checks: bm_words follows the bitmap verify's rule — any value up to 0xFFFFFFFF, 0 included (part_bits and signer_bits may then be
 * NULL); keys beyond the bitmap are absent, bits beyond the key set give 2; else BN254_E_BAD_ARGUMENT.  n and n_parts < 2^32.  Host form:
 * part_off[0] == 0, non-decreasing, part_off[n] == n_parts.  BN254_E_MISALIGNED as in the collect: parts, part_bits, agg_sigs, signer_bits and
 * n_signers 4-byte aligned, the offsets 8-byte aligned.  n == 0 returns 0.  BN254_OPT_MAX_CHUNK slices the PARTIALS (and the tuples' hashing),
 * as the collect slices shares; the outputs are the same.
 * Security: a proof of possession of every registered key is assumed, as in the rest of the family.
 * Cost: ONE hash-to-G1 per tuple; per partial the bitmap verify's aggregate key (subset tables: n_keys / 8 additions) and one verify; then a
 * select-and-sum launched once behind the last slice, in two layouts chosen per tuple by its number of partials: below
 * BN254_OPT_MERGE_WAVE_MIN_PARTS one lane walks the tuple (all bm_words words of each partial's row, one addition per taken partial); from
 * there on a wave does — lane l owns words l, l + 64, .. of the row, one wave vote per status-0 partial decides, then the 64 lanes add the
 * taken partials l, l + 64, .. and six levels of additions in LDS fold the partial sums.  All additions are complete.  The _device form only
 * enqueues: no host synchronisation, the range rule included.
 * Profiling: bn254_ctx_last_kernel_ms keeps four intervals with the exact collect's meaning: ms[0] front end (hash once per tuple, decode,
 * spread, aggregate keys), ms[1] select-and-sum (it runs last), ms[2] Miller loop, ms[3] final exponentiation — of the last slice.
 * Which call when: this one wherever a node holds partial aggregates per message; the route without it is
 * bn254_batch_verify_keyed_bitmap_device on the repeated messages, a copy of the statuses to the host, the first-fit filter there, and
 * bn254_batch_g1_sum.  Measured on an MI355X (tools/merge_throughput.py, profiles/merge_throughput.jsonl; 256 keys, two thirds signing in
 * disjoint committees, every partial valid, whole-call medians of 9 alternating calls on a caller's stream, inputs resident, min .. max in
 * brackets): 256 tuples x 16 partials 3.07 ms [3.05 .. 3.09] against that route's 3.50 [3.49 .. 3.51]; 4 096 x 4 5.14 [5.09 .. 5.17] against
 * 5.88 [5.83 .. 5.93]; 1 024 x 64 11.8 [11.6 .. 12.5] against 15.3 [15.0 .. 16.3]; one tuple of 4 096 one-bit partials 4.21 [4.19 .. 4.26]
 * against 6.64 [6.28 .. 7.08] — the call is ahead beyond the spread at all four, by 1.14 x to 1.58 x.  The other route's interval holds its
 * host filter (numpy: 0.22, 0.65, 2.9 and 0.73 ms of it); with the filter's time taken off entirely the call is still ahead at every shape
 * (3.07 against 3.28, 5.14 against 5.23, 11.8 against 12.4, 4.21 against 5.91).  Per stage (front end, select-and-sum, Miller loop, final exponentiation): 256 x 16 0.71 + 0.23 + 1.04 + 1.13
 * ms; 1 024 x 64 1.39 + 0.41 + 6.06 + 3.90; the lone tuple 0.36 + 1.59 + 1.07 + 1.14 — there the select, serial in 4 096 partials for one
 * wave, costs 0.39 us per partial and is the largest stage; the collect sums the same shares in 0.27 ms, so a caller whose partials are all
 * single shares takes the collect.  No shape at which the call loses was found; shapes with invalid partials were not measured.
 * The optimistic form (one verify of the tuple's sum when its partials are pairwise disjoint) is bn254_batch_merge_keyed_bitmap_optimistic,
 * below.  Compressed partials: BN254_FLAG_G1_COMPRESSED (33 bytes per partial, no alignment).  Out of scope: a randomised form, the multi-GPU layer. */
int bn254_batch_merge_keyed_bitmap(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */,
                                   const uint8_t *parts /* n_parts*64 */, const uint32_t *part_bits /* n_parts*bm_words */,
                                   const uint64_t *part_off /* n+1 */, size_t n_parts, size_t n, size_t bm_words, uint32_t flags,
                                   uint8_t *part_status /* n_parts */, uint8_t *part_taken /* n_parts */, uint8_t *tuple_status /* n */,
                                   uint8_t *agg_sigs /* n*64 */, uint32_t *signer_bits /* n*bm_words */, uint32_t *n_signers /* n, or NULL */);
int bn254_batch_merge_keyed_bitmap_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_parts,
                                          const uint32_t *d_part_bits, const uint64_t *d_part_off, size_t n_parts, size_t n, size_t bm_words,
                                          uint32_t flags, uint8_t *d_part_status, uint8_t *d_part_taken, uint8_t *d_tuple_status,
                                          uint8_t *d_agg_sigs, uint32_t *d_signer_bits, uint32_t *d_n_signers, void *stream);

/* bn254_batch_merge_keyed_bitmap_optimistic[_device]: the exact merge's arguments and six outputs, with ONE verify per tuple.  The partials
 * of a tuple share the message: if every candidate is good and their rows are pairwise disjoint, their sum is the aggregate of the union row,
 * and
 *     e(H(m_i), sum_{j in union row} pk_j) * e(sum of the taken sigma, -G2) == 1
 * proves it.  Only a tuple whose sum fails, or that holds an overlap, needs its partials checked one by one.  No randomness, no seed.  The
 * argument checks, BN254_E_MISALIGNED, the range rule, the fills (part_status with 2, part_taken with 0) and the _device conventions are those
 * of bn254_batch_merge_keyed_bitmap[_device]: no host synchronisation, every buffer reserved before the first kernel, everything enqueued
 * whether or not a tuple fails; BN254_OPT_MAX_CHUNK slices the partials (of the fallback) and the tuples (of the hash and of the tuple check).
 *   1. PRE-CHECK.  Every partial of an accepted tuple gets rules 1-3 of identity 1, in that order and with the call's flags: sigma's decode
 *      status; the status of the lowest bad bit of its row; the tuple's hash status.  No pairing and no aggregate key is computed.  Status 0
 *      means the partial is a CANDIDATE.  A candidate may have an empty row.
 *   2. PROVISIONAL SELECT.  The exact call's first fit, run over the pre-check statuses in both layouts.  It additionally reports an
 *      OVERLAP: a candidate refused because its row meets the union taken so far.
 *   3. FLAG PER TUPLE, decided on the device.  FINAL: no candidate — by the number of candidates, not by the popcount of the row, because an
 *      empty-row candidate still needs its check.  EXACT: an overlap was reported.  CHECK: everything else, i.e. every candidate was taken.
 *   4. TUPLE CHECK.  For every CHECK tuple one verify e(H(m_i), sum_{j in union row} pk_j) * e(sum of the taken sigma, -G2) == 1, over the
 *      call's own outputs through the bitmap verify's kernels, with decode flags 0 — an identity sum is legitimate.  It runs over all n tuples
 *      in pieces of the slicing rule's size; the verdicts of tuples that are not CHECK are not read.
 *   5. PASS.  The provisional row, aggregate, count, part_taken and statuses are final.
 *   6. FALLBACK.  The candidates of the tuples that fail the check or are EXACT are queued on the device and verified exactly as the bitmap
 *      verify would: the aggregate key per queued partial, the Miller loop and the final exponentiation over the queue only (every partial
 *      of a slice is still decoded and spread).  The tuples' rows are zeroed and the exact first-fit select-and-sum runs again for these
 *      tuples only; it rewrites part_taken for all of their partials.  Their six outputs are byte for byte the exact merge's.  A passing
 *      tuple's outputs are not touched by the re-select.
 *   7. WHOLE-CALL ROUTING.  The call IS the exact merge (same bytes) when no keys are registered, when BN254_OPT_PAIR_LANES is off (the
 *      queue's kernels are lane-pair kernels), or when n_parts < BN254_OPT_MERGE_OPT_MIN_PARTS.  There is no per-tuple minimum: the collect's
 *      measurements showed that such an option only pushes tuples through the queue, and a one-candidate tuple's check is the exact verify
 *      anyway.
 * IDENTITY 2 OF THE MERGE HOLDS UNCONDITIONALLY: bn254_batch_verify_keyed_bitmap with flags 0 on the call's own outputs returns 0 for every
 * tuple with tuple_status == 0 — a passing tuple has just been verified so, a fallback tuple is the exact call's, a FINAL one is empty.
 * EQUALITY WITH THE EXACT CALL: all six outputs equal bn254_batch_merge_keyed_bitmap's whenever no passing tuple holds a candidate that the
 * exact call would have given 9.
 * THE ONE DEVIATION: candidates whose errors cancel inside a passing tuple — sigma_a + D and sigma_b - D, also with empty rows — read 0 and
 * are taken; the exact call gives both 9.  The aggregate is still the valid one for the union row.  A caller who needs per-partial verdicts
 * uses the exact call.  Identity 1 holds only up to this deviation.
 * With one-bit rows and distinct keys per tuple the outputs equal bn254_batch_collect_keyed_bitmap_optimistic's (part_status as its
 * share_status).
 * Cost: with every partial valid the aggregate keys, the Miller loop and the final exponentiation run over n tuples instead of n_parts
 * partials; per partial remain the decode and rule 2 of the pre-check, one G1 addition, and the decode and spread of the fallback's front
 * end, which runs whether or not anything is queued.  With every tuple failing the call costs the exact call plus one n-item verify pass.
 * Which call when (measured on an MI355X, tools/merge_throughput.py --optimistic, profiles/merge_throughput.jsonl: whole-call medians of 9
 * alternating calls after two warm-ups on a caller's stream, inputs resident, 256 keys, two thirds signing in disjoint committees, min .. max
 * in brackets).  Every partial valid: 256 tuples x 16 partials 1.84 ms [1.84 .. 1.86] against the exact merge's 3.10
 * [3.09 .. 3.16]; 4 096 x 4 2.95 [2.95 .. 2.96] against 5.10 [5.07 .. 5.15]; 1 024 x 64 2.53 [2.51 .. 2.54] against 11.9 [11.8 .. 12.0]
 * (4.7 x); 64 x 16 1.84 against 2.43; 16 x 16 1.81 against 1.93; 8 x 16 1.82 against 1.92; 4 x 16 1.81 [1.79 .. 1.82] against 1.86 [1.86 ..
 * 1.88] — ahead beyond the spread from 64 partials on; 2 x 16 (1.81 against 1.82) and 1 x 16 (1.82 against 1.80) tie.  The call is one verify
 * pass of n items plus 0.9 ms whatever the partials: per stage 256 x 16 0.41 + 0.37 + 0.98 + 0.08 ms, 4 096 x 4 0.42 + 0.37 + 2.09 + 0.09,
 * 1 024 x 64 0.61 + 0.38 + 1.46 + 0.09 — ms[2] is a bitmap verify's Miller loop and final exponentiation at n items (0.98 ms up to 256, 1.46 at
 * 1 024, 2.09 at 4 096), as the optimistic collect found.  ANY tuple that goes the exact way costs the call one pass of the queue's lane-pair
 * kernels (aggregate keys, Miller loop, final exponentiation), 6.3 - 7.6 ms here whether it queues 4 partials or 656: one failing tuple takes
 * 256 x 16 to 8.62 ms [8.15 .. 9.47] against the exact merge's 3.18, 4 096 x 4 to 9.33 against 5.67, 16 x 16 to 9.05 against 1.91, and 1 024 x
 * 64 to 8.92 against 12.8 (still ahead); 1 % wrong partials spread over the call: 256 x 16 (41 tuples fail) 8.72 against 3.18, 4 096 x 4 (164)
 * 9.45 against 5.67, 1 024 x 64 (655 tuples, 41 920 partials queued) 13.3 against 12.1 — the exact call plus the optimistic pass.  A tuple whose
 * candidates OVERLAP sends itself the exact way: one tuple of 4 096 one-bit partials over 256 keys takes 10.4 ms against 4.21 (both selects
 * are serial in the partials: 1.7 ms each).  So: this call where partials are disjoint and almost all valid and the call has 64 partials or
 * more (BN254_OPT_MERGE_OPT_MIN_PARTS); the exact call for per-partial verdicts, for overlapping partials (single shares belong to the
 * collect), and where a failing tuple is expected in a call the exact route serves in under 8 ms.  The exact merge is unchanged by the
 * route: against the parent commit's build in the same process, alternating, -1.8 % .. +0.1 % over the ten shapes (the parent's own calls
 * spread -1.5 % .. +1.8 % about their median).  Not measured: between 32 and 64 partials, tuples of other lengths than 4, 16 and 64 below 256
 * tuples, key sets other than 256 keys, wrong partials beyond the four shapes named.
 * Profiling: ms[0] = front end (hash, range rule, pre-check) and provisional select-and-sum, ms[1] = aggregate keys of the union rows, ms[2] =
 * the tuples' Miller loop and final exponentiation, ms[3] = fallback and re-select.
 * Compressed partials: BN254_FLAG_G1_COMPRESSED.  Out of scope: a short queue served by the small-batch kernels, a randomised merge, the multi-GPU layer. */
int bn254_batch_merge_keyed_bitmap_optimistic(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */,
                                              const uint8_t *parts /* n_parts*64 */, const uint32_t *part_bits /* n_parts*bm_words */,
                                              const uint64_t *part_off /* n+1 */, size_t n_parts, size_t n, size_t bm_words, uint32_t flags,
                                              uint8_t *part_status /* n_parts */, uint8_t *part_taken /* n_parts */, uint8_t *tuple_status /* n */,
                                              uint8_t *agg_sigs /* n*64 */, uint32_t *signer_bits /* n*bm_words */,
                                              uint32_t *n_signers /* n, or NULL */);
int bn254_batch_merge_keyed_bitmap_optimistic_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_parts,
                                                     const uint32_t *d_part_bits, const uint64_t *d_part_off, size_t n_parts, size_t n,
                                                     size_t bm_words, uint32_t flags, uint8_t *d_part_status, uint8_t *d_part_taken,
                                                     uint8_t *d_tuple_status, uint8_t *d_agg_sigs, uint32_t *d_signer_bits, uint32_t *d_n_signers,
                                                     void *stream);

/* PROOFS OF POSSESSION — what every same-message aggregate call above assumes of the registered keys (the bitmap verify and its randomised
 * form, the three collect calls, the two merge calls, the distinct-message keyed calls).  Without one, an attacker who registers
 * pk* = a G2 - pk_v makes the aggregate key of {victim, attacker} equal a G2 and forges "both signed m" as a H(m) without the victim's
 * secret.  The reference names the remedy (src/lib.rs:34-38): each key holder proves possession "by signing a message".
 * THE SCHEME.  BN254_POP_TAG is 16 ASCII bytes.  The proof message of a key is TAG || pk: the tag, then the 128 bytes of the key's
 * uncompressed G2 encoding EXACTLY as the caller passes them — 144 bytes.  It is hashed by the library's one hash-to-G1 (try-and-increment,
 * src/hash.rs:29-63).  The proof is pop = sk * H(TAG || pk), a 64-byte uncompressed G1 point — ECDSA::sign (src/ecdsa.rs:26-35) on that
 * message — and it is checked as e(H(TAG || pk), pk) * e(pop, -G2::one()) == 1 — ECDSA::verify (src/ecdsa.rs:49-64).
 * TWO CALLER RULES.  The reference's hash has no domain separation (src/hash.rs:30-33), so the tag separates proofs from signatures only
 * if the caller keeps them apart:
 *   1. a signer must REFUSE application messages that begin with BN254_POP_TAG — a signature on TAG || pk' is a proof for pk';
 *   2. a proof is bound to the key's ENCODING BYTES: the bytes hashed are the bytes passed, so a key must be presented to the verifier in
 *      the encoding it was proven in (the uncompressed encoding of a curve point is unique; an encoding with a coordinate >= q is refused).
 * DEFINING IDENTITIES, byte for byte.
 *   bn254_batch_pop_prove[_device]: pks = what bn254_batch_g2_mul(NULL, sks, reduce_scalar = 1) gives; pops[i] = what bn254_batch_sign
 *     gives for the message TAG || pks[i] and sks[i]; status[i] = the first non-zero status of the two (the key derivation's, then the
 *     signature's: 1 HashToPointError is the only one either can give).  Pinned: a scalar >= r is reduced mod r by both steps (Fr::from_slice),
 *     so sk and sk mod r give the same bytes; sk == 0 (mod r) gives the identity twice — pk and pop all-zero bytes, status 0.  That pair
 *     verifies under flags = 0 (e(H, O) * e(O, -G2) == 1) and reports 4 under BN254_FLAG_REJECT_IDENTITY: a verifier of proofs passes that flag.
 *   bn254_batch_pop_verify[_device]: status[i] = the status of bn254_batch_verify on message TAG || pk_i, signature pop_i, key pk_i under
 *     flags | BN254_FLAG_G2_SUBGROUP_CHECK (a proof for a key outside the order-r subgroup means nothing).  Status order as there: the
 *     proof's decode status, the key's, the hash status, then 0 or 9.
 *   bn254_ctx_register_keys_pop: key_status[j] (may be NULL) = what bn254_ctx_register_keys reports for key j if that is non-zero, else what
 *     bn254_batch_pop_verify reports for (pk_j, pop_j) under flags & BN254_FLAG_REJECT_IDENTITY.  THAT BYTE BECOMES THE KEY'S REGISTRATION
 *     STATUS: every keyed call reads it where it read the plain registration's, so a key whose proof failed is refused with 9 by
 *     bn254_batch_verify_keyed, by rule 2 of the bitmap verify (the lowest bad bit) and its randomised form, by the collect, merge and
 *     distinct-message keyed calls — while the proven keys verify.  Otherwise the call is bn254_ctx_register_keys: it replaces the key set,
 *     waits as that call does, invalidates the bitmap call's bad-bit vector and subset tables, is synchronous (statuses and tables are final
 *     when it returns), and bn254_ctx_register_keys afterwards registers plainly again.
 *     FAIL CLOSED: if anything after the keys' own registration step fails (a HIP error, an allocation), the context is left with NO keys
 *     registered — never with keys in place whose proofs were not checked.  Argument errors (pops == NULL with n_keys > 0 included) return
 *     BN254_E_BAD_ARGUMENT before anything is touched: the previous set stays.
 *     Cost: the plain registration, then on the same stream a composer kernel (TAG || pk_j from the staged keys: no second copy of the
 *     keys crosses the bus), the decode of the proofs, the hash of the messages and ONE keyed verify per key against the key's own freshly
 *     built line table, on the routing-table row of n_keys items; a fold kernel writes the statuses.
 * These calls take no message buffer: a pending bn254_ctx_expect_msgs_len is neither consumed nor applied (the composed buffer is bounded by
 * its true length) and stays armed for the caller's next hashing call.  _device forms: d_sks, d_pks, d_pops 4-byte aligned, else
 * BN254_E_MISALIGNED; they only enqueue (the first key derivation of a context builds its fixed-base table synchronously, as
 * bn254_batch_g2_mul_device does); BN254_OPT_MAX_CHUNK and the workspace rule slice them as they slice a verify.  n < 2^32.
 * bn254_ctx_register_pools takes raw pools, not registered keys: proofs for pooled keys are out of scope (check them with
 * bn254_batch_pop_verify first).  Measured cost of the three calls: DESIGN.md section 10j. */
#define BN254_POP_TAG "BN254G2_POP_V01:"
#define BN254_POP_TAG_LEN 16
int bn254_batch_pop_prove(bn254_ctx *ctx, const uint8_t *sks /* n*32 */, size_t n, uint8_t *pks /* n*128 */, uint8_t *pops /* n*64 */,
                          uint8_t *status /* n */);
int bn254_batch_pop_prove_device(bn254_ctx *ctx, const uint8_t *d_sks, size_t n, uint8_t *d_pks, uint8_t *d_pops, uint8_t *d_status, void *stream);
int bn254_batch_pop_verify(bn254_ctx *ctx, const uint8_t *pks /* n*128 */, const uint8_t *pops /* n*64 */, size_t n, uint32_t flags,
                           uint8_t *status /* n */);
int bn254_batch_pop_verify_device(bn254_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pops, size_t n, uint32_t flags, uint8_t *d_status,
                                  void *stream);
int bn254_ctx_register_keys_pop(bn254_ctx *ctx, const uint8_t *pks /* n_keys*128 */, const uint8_t *pops /* n_keys*64 */, size_t n_keys,
                                uint32_t flags, uint8_t *key_status /* n_keys or NULL */);

/* THRESHOLD SIGNATURES over the registered keys: t-of-n BLS.  The group key is Shamir-shared by a polynomial f of degree t - 1; registered
 * key j is pk_j = f(j + 1) * G2::one() — key index j stands for the evaluation point x_j = j + 1, so index 0 is a legal signer — and validator
 * j's share of a message is the ordinary signature under pk_j.  Any t valid shares interpolate to THE signature under f(0) * G2::one(), which
 * bn254_batch_verify (or one pairing check on chain) accepts under the group key.  This call checks the shares and interpolates.
 * Inputs, argument checks, alignment rules, the range rule of the _device form, the fill of share_status with 2, BN254_OPT_MAX_CHUNK slicing
 * and bn254_ctx_expect_msgs_len are exactly those of bn254_batch_collect_keyed_bitmap[_device] above; in addition threshold == 0 is
 * BN254_E_BAD_ARGUMENT.  A threshold above n_keys is legal: every accepted tuple then fails as described below.
 * share_status[s], DEFINING IDENTITY 1: the collect's — byte for byte what bn254_batch_verify_keyed returns, with the same flags, for
 * n_shares items whose message is their tuple's message repeated (the call runs the collect's front end and verify slices as they stand).
 * Let V_i be the set of key indices with at least one status-0 share in accepted tuple i (the collect's bitmap row); n_valid[i] = |V_i| (the
 * array may be NULL).
 *   |V_i| >= threshold: S_i = the `threshold` LOWEST indices of V_i — a choice that depends on nothing but V_i, so the bytes do not depend on
 *     the order of the shares, on slicing or on the layout of the sum.  used_bits row i = S_i (exactly `threshold` bits, in the bitmap call's
 *     numbering), group_sigs[i] = sum over j in S_i of lambda_j(S_i) * sigma_j, where sigma_j is a status-0 share of key j (several are the
 *     same point: bn254_batch_collect_keyed_bitmap) and lambda_j(S) = prod x_k / prod (x_k - x_j) over the k != j of S, mod r.  Uncompressed,
 *     the identity as 64 zero bytes.  tuple_status[i] = 0.
 *   |V_i| < threshold: tuple_status[i] = 9 (VerificationFailed), group_sigs[i] = 64 zero bytes, used_bits row i = V_i — who is there.
 *   A tuple the range rule refuses reads 2, one whose hash status is non-zero reads that status (in the collect's order); both get the empty
 *     row, 64 zero bytes and n_valid 0.
 * DEFINING IDENTITY 2: group_sigs[i] is byte for byte bn254_batch_g1_msm of the chosen shares with the coefficients above.
 * DEFINING IDENTITY 3 (closed loop, flags = 0): for registered keys pk_j = f(j + 1) * G2::one() of ONE polynomial of degree threshold - 1,
 * bn254_batch_verify of (m_i, group_sigs[i], f(0) * G2::one()) returns 0 for every tuple with tuple_status 0, whatever subset signed, and
 * group_sigs[i] is the same point for every subset.
 * WHAT IS CHECKED: every share against its registered key.  WHAT IS NOT, by this call: that the registered keys lie on one polynomial of
 * degree threshold - 1 — producing such a set is the dealer's or the DKG's job, and bn254_ctx_check_dealing below is the call with which a
 * committee checks the set it was handed, once per key set.  For a key set that does not, the output is still well defined (the rule for
 * S_i) but is the signature of no key in particular.  Registration statuses apply as in every keyed call (a key registered with a failed proof
 * of possession has no valid share).
 * Cost: the collect's — one hash per tuple, one keyed verify per share, its select-and-sum — then a lane per tuple for rank and select (the
 * `threshold` lowest bits of the row, counted across its words), a lane per share that claims its kept key and writes the key's
 * coefficient (2 (t - 1) products and one inversion in Fr: about 2t + 400 products), and bn254_batch_g1_msm's term and sum kernels over
 * ALL the shares, masked: a lane whose share is not kept walks the identity, and every wave that holds at least one kept share walks the
 * full 128-step ladder.  Scratch beyond the collect's: 142 B per share and a second bitmap row per tuple.  The _device form only
 * enqueues: no host synchronisation.  Under bn254_ctx_set_profiling the intervals are the collect's, with the interpolation inside ms[1] (select-and-sum).
 * Measured on an MI355X (tools/threshold_throughput.py, profiles/threshold_throughput.jsonl; 256 keys, every share valid, threshold = two
 * thirds of a tuple's keys; _device forms under HIP events, median [min, max] of 7): 256 tuples x 171 shares 11.42 ms [11.31, 11.52] against
 * 8.28 [8.23, 8.36] for bn254_batch_collect_keyed_bitmap_device on the same inputs; 4 096 x 11: 11.10 against 8.32; one tuple of 4 096
 * shares: 6.13 against 2.74.  So the interpolation costs 2.8 - 3.4 ms — a ladder per kept share is what bn254_batch_g1_mul costs, and one
 * ladder is about 3 ms of latency however few lanes walk one; it is a third on top of the verification, not a small addition.  The route
 * without the call (keyed verify, statuses to the host, coefficients in Python integers, g1_mul, g1_sum): 654.5, 76.4 and 11.8 ms, the
 * same signature bytes.  Unmeasured: other thresholds, invalid shares, more than 256 keys, the host form.
 * Which call when: this one whenever the shares are in hand and the share keys registered; bn254_batch_collect_keyed_bitmap for
 * multi-signatures (no interpolation); bn254_batch_g1_msm for weighted sums of the caller's own points.  DESIGN.md section 10k.
 * Compressed shares: BN254_FLAG_G1_COMPRESSED.  Out of scope: a randomised form, the multi-GPU layer, and PRODUCING a dealing in the C ABI (Shamir sharing, the
 * rounds of a DKG, checks of shares against commitments; bn254_batch_g2_msm is the building block for sum x^k C_k).  No longer out of
 * scope: checking a dealt key set (bn254_ctx_check_dealing), and an optimistic form that interpolates first and verifies the result once — bn254_batch_threshold_combine_keyed_optimistic below. */
int bn254_batch_threshold_combine_keyed(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */,
                                        const uint8_t *shares /* n_shares*64 */, const uint32_t *share_key /* n_shares */,
                                        const uint64_t *share_off /* n+1 */, size_t n_shares, size_t n, size_t bm_words, uint32_t threshold,
                                        uint32_t flags, uint8_t *share_status /* n_shares */, uint8_t *tuple_status /* n */,
                                        uint8_t *group_sigs /* n*64 */, uint32_t *used_bits /* n*bm_words */, uint32_t *n_valid /* n, or NULL */);
int bn254_batch_threshold_combine_keyed_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_shares,
                                               const uint32_t *d_share_key, const uint64_t *d_share_off, size_t n_shares, size_t n,
                                               size_t bm_words, uint32_t threshold, uint32_t flags, uint8_t *d_share_status,
                                               uint8_t *d_tuple_status, uint8_t *d_group_sigs, uint32_t *d_used_bits, uint32_t *d_n_valid,
                                               void *stream);

/* THE GROUP KEY of the optimistic threshold call below: f(0) * G2::one(), the key the consumer of a group signature checks it under.
 * group_pk = 128 bytes, decoded and tabulated exactly as one key of bn254_ctx_register_keys is (same flags, same status codes; the
 * identity, 128 zero bytes, is a legal group key as it is a legal registered key), into a one-entry table of its own; NULL forgets the key.
 * A non-zero decode status is reported in *status (may be NULL) and leaves NO group key set; the call itself returns 0.  Quiesces the
 * context first, like a registration.  LIFETIME: bn254_ctx_register_keys and bn254_ctx_register_keys_pop forget the group key — a new key
 * set is a new dealing.  This call does NOT check that the registered keys interpolate to this key — bn254_ctx_check_dealing below computes
 * the key they do interpolate to —: a key that does not belong to the set sends every tuple of the optimistic call the exact way (slower, the exact call's bytes) and can never make a wrong signature pass,
 * because what passes has verified under the key the caller named. */
int bn254_ctx_set_group_key(bn254_ctx *ctx, const uint8_t *group_pk /* 128, or NULL: forget it */, uint32_t flags, uint8_t *status /* 1, or NULL */);

/* CHECK A DEALING: are the registered keys 0 .. n - 1 (n = the number registered, key j standing for x_j = j + 1) a t-of-n dealing — do they
 * lie on ONE polynomial of degree below t = threshold — and which group key do they interpolate to.  What a committee runs once on the key
 * set a dealer or a DKG round handed it, before the threshold calls above are worth anything.  Host-synchronous: like a registration it
 * quiesces the context first and returns after the outputs are written.  It does NOT install the group key (bn254_ctx_set_group_key does).
 * BN254_E_BAD_ARGUMENT: threshold == 0, no registered keys, flags != 0, a NULL seed32, group_pk or status.  Otherwise four outcomes, tested
 * in this order (bad_key may be NULL):
 *   1. a key has a non-zero registration status (decode fault, failed proof of possession): *status = that status, the LOWEST such key
 *      wins, *bad_key = its index, group_pk = 128 zero bytes; nothing else is computed.
 *   2. threshold > n: *status = 9, *bad_key = UINT32_MAX, group_pk zeroed; nothing else is computed.
 *   3. the degree check fails: *status = 9, *bad_key = UINT32_MAX, group_pk zeroed.
 *   4. it passes: *status = 0, *bad_key = UINT32_MAX, group_pk = K.  With threshold == n there is nothing to check: 0 and K.
 * K = sum over k < t of lambda_k pk_k, lambda_k the coefficients bn254_debug_lagrange_at_zero gives for the points 1 .. t.  DEFINING IDENTITY:
 * K is byte for byte bn254_batch_g2_msm of the first t keys' uncompressed bytes under those scalars.
 * THE DEGREE CHECK is randomised.  rho_j, for j in [t, n), is the 128-bit weight of index j under seed32 — the first 16 bytes of
 * SHA-256(seed32 || le64(j)) read little-endian, 0 mapped to 1: the derivation of bn254_batch_verify_randomized.  c_j = rho_j for j >= t, and
 * c_k = -sum over j in [t, n) of rho_j L_k(x_j) mod r for k < t, L_k(x) = prod over i < t, i != k of (x - x_i) / (x_k - x_i).  The keys pass
 * iff sum over j < n of c_j pk_j is the identity: key j >= t contributes rho_j (pk_j - the value the first t keys interpolate at x_j).
 * For a true dealing the sum is the identity under EVERY seed, so a 9 is always exact.  A 0 is wrong with probability <= 2^-128, PROVIDED
 *   (a) the seed is fresh and unpredictable to whoever produced the keys (drawn after the keys were fixed), and
 *   (b) the keys are in the order-r subgroup: they were registered with BN254_FLAG_G2_SUBGROUP_CHECK.
 * Which keys are off the polynomial is not reported.
 * Cost: the coefficients on the device in Fr — the points are consecutive, so every product of differences is a factorial: a table of
 * factorials (one wave, a product scan), a table of the inverses of 1 .. n (one inversion per entry, a lane each), then a lane per k < t
 * walking the j: (n - t) products and one inversion — O(t (n - t)) products and O(n) inversions in all.  Then K and the check as ONE launch
 * of bn254_batch_g2_msm's kernels over two segments, t + n terms, whose term kernel reads the registered keys' table instead of decoding
 * bytes; a last kernel settles the verdict, and the host reads 128 + 4 + 1 bytes.  Under bn254_ctx_set_profiling: ms[0] key scan and
 * coefficients, ms[1] terms, ms[2] sums, ms[3] verdict.
 * Measured on an MI355X (tools/dealing_throughput.py, profiles/dealing.jsonl; keys dealt from one polynomial and registered; whole calls
 * under a host clock, median [min, max] of 7): n = 256, t = 171: 7.04 ms [7.03, 7.15] against 16.06 [15.95, 18.47] for the Python-integer
 * route (the same closed-form coefficients in Python integers, then bn254_batch_g2_mul and bn254_batch_g2_sum over the t + n products) and
 * 30.3 [29.3, 35.4] for the exact route ((n - t) t = 14 535 products, each key j >= t compared with its interpolation); 1 024, 683: 7.98
 * [7.92, 8.01] against 69.2 [66.0, 79.1]; 4 096, 2 731: 11.48 [11.42, 11.59] against 593 [574, 599].  Stages of ONE profiled call
 * (coefficients, terms, sums): 1.76, 4.99, 0.35 ms at 256; 2.32, 5.02, 0.63 at 1 024; 4.57, 5.03, 1.96 at 4 096 — a 256-step G2 ladder is
 * 5 ms of latency however few lanes walk one, and at 4 096 keys the lane per k that walks 1 365 products and an inversion takes as long.
 * Unmeasured: other thresholds, key sets that fail (the same work), more than 4 096 keys.
 * DESIGN.md section 10m.  Out of scope: the multi-GPU layer, compressed keys, locating the keys that are off, 64-bit weights, a bucket-method sum. */
int bn254_ctx_check_dealing(bn254_ctx *ctx, uint32_t threshold, const uint8_t *seed32 /* host */, uint32_t flags /* must be 0 */,
                            uint8_t *group_pk /* 128 */, uint8_t *status /* 1 */, uint32_t *bad_key /* 1, or NULL */);

/* EVALUATE COMMITMENT VECTORS: p polynomials with G2 coefficients (lowest degree first; polynomial i is the coefficients
 * [poly_off[i], poly_off[i+1]) of the m = poly_off[p] given) and q evaluations; evaluation e is the pair (polynomial eval_poly[e], point
 * eval_x[e]), x any uint32:  out[e] = sum over k of x^k C_k, with 0^0 = 1, so x = 0 returns C_0.  What a committee does with the t Feldman
 * commitments C_k = a_k G2 a dealer or a DKG round hands it: pk_j = f(j + 1) G2 for its n validators, and the check of a received share
 * against a dealer's vector (secret * G2 == the vector at index + 1).
 * DEFINING IDENTITY: out[e] and status[e] are byte for byte bn254_batch_g2_msm over ONE segment holding that polynomial's coefficients, with
 * the scalars x^k mod r as 32 big-endian bytes and reduce_scalar = 0.  So: coefficients are decoded with flags 0 (on the curve, NO subgroup
 * check); the first non-zero decode status in coefficient order wins and the output is then 128 zero bytes; an empty polynomial gives the
 * identity with status 0; the identity is a legal coefficient.  In addition eval_poly[e] >= p reads status 2 with the identity, and in the
 * _device form so does a polynomial whose offsets are reversed or run past d_poly_off[p], with no read outside the buffers; a fault in one
 * polynomial touches only the evaluations that name it.  (The identity is one of group elements of order r.  For a coefficient OUTSIDE the
 * order-r subgroup — legal under flags 0 — it holds while x^k < r, i.e. where x^k mod r is x^k; beyond that Horner's rule multiplies by the
 * integer x where the identity's scalar was reduced, and the result is the layout's.  A key made of such coefficients is judged by the
 * registration's own subgroup check, below.)
 * Argument checks and alignment are those of bn254_batch_g2_msm: p, q < 2^32, at most 2^32 - 1 coefficients; host form: poly_off
 * non-decreasing, else BN254_E_BAD_ARGUMENT; _device form: d_poly_off 8-byte aligned, d_coeffs, d_eval_poly, d_eval_x and d_out 4-byte
 * aligned, else BN254_E_MISALIGNED.  As there the _device form copies d_poly_off[p] home to size its scratch (146 B per coefficient): ONE
 * 8-byte copy and a wait for the stream before anything is enqueued, so it cannot be captured into a graph.  One call per context in flight.
 * Cost: the coefficients are decoded ONCE (a lane each), not once per evaluation.  An evaluation of a polynomial of fewer than
 * BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS coefficients is one lane's Horner walk from the top coefficient, acc <- x acc + C_k: per coefficient
 * one doubling per bit of x, one complete addition per set bit, one mixed addition — about 20 group operations for a 9-to-13-bit x where a
 * 256-step ladder spends about 320 —, the loop bounds those of the longest polynomial and the widest x in the wave.  A longer polynomial is
 * a wave's: lane c walks the chunk [c L, (c+1) L), L = ceil(len / 64), multiplies its partial by x^(c L) mod r (Fr on the device, then the
 * 256-step ladder over the partial brought to affine form) and the six-level tree of the sums folds the 64 products; one inversion per
 * evaluation in either layout, and one per lane in the wave layout.
 * Measured on an MI355X (tools/poly_eval_throughput.py, profiles/poly_eval.jsonl; whole calls under a host clock, staging on both sides, median
 * [min, max] of 7 alternating runs after 2 warm-up runs; the baseline is the route that exists without the call: the scalars x^k mod r in
 * Python integers, then bn254_batch_g2_msm over n segments of t terms, each part timed): the share keys of n = 256, t = 171: 6.11 ms [6.03,
 * 6.11] against 5.89 [5.85, 6.09] for the scalars + 7.09 [6.86, 7.23] for g2_msm; 1 024, 683: 12.4 [11.3, 28.3] against 98.1 + 73.5
 * [73.4, 75.0]; 4 096, 2 731: 109.8 [109.5, 110.3] against 1 550 + 1 193 — the baseline there was run on the first 256 keys and SCALED by 16
 * (in full it stages 1.4 GB of points).  The _device form under events: 5.96, 11.09 and 107.4 ms.  64 polynomials of 171 coefficients at
 * one 13-bit x (the share check of a DKG round): 5.83 [5.82, 5.83] against 1.50 + 5.49 [5.48, 5.51] — bn254_batch_g2_msm ALONE is 0.3 ms
 * faster there, outside both spreads; this call wins only by the scalars it does not need.  Which call when: this one for evaluation points
 * below 2^32 — it needs no scalars, stages every coefficient once and its scratch is 146 B per coefficient, not 217 B per term —;
 * bn254_batch_g2_msm for scalars that are not powers of a small integer, and, where the scalars are at hand already, for a few dozen
 * evaluations of polynomials of about 171 coefficients, where the two are within 6 %.  bn254_ctx_register_keys_commitments against
 * evaluation, keys home, bn254_ctx_register_keys: 13.36 [13.35, 13.38] against 13.46 [13.42, 13.48] at (256, 171), 19.54 against 19.68
 * (spreads overlap) at (1 024, 683), 116.96 against 116.95 at (4 096, 2 731): a tie — the registration's own line tables are the cost, the
 * round trip of 128 B per key is not; what the call saves is the host's part.  bn254_batch_g2_msm (171 terms) and bn254_ctx_check_dealing
 * (256, 171) in this build against the parent's: 5.40 and 7.04 ms against 5.39 and 7.08, within the spreads.
 * Unmeasured: other thresholds, more than 4 096 keys, x wider than 13 bits at scale, the multi-GPU layer.
 * DESIGN.md section 10n.  Out of scope: the multi-GPU layer, compressed commitments, a G1 form, non-integer or 256-bit evaluation points, a
 * forward-difference scheme for consecutive points. */
int bn254_batch_g2_poly_eval(bn254_ctx *ctx, const uint8_t *coeffs /* m*128 */, const uint64_t *poly_off /* p+1 */, size_t p,
                             const uint32_t *eval_poly /* q */, const uint32_t *eval_x /* q */, size_t q, uint8_t *out /* q*128 */,
                             uint8_t *status /* q */);
int bn254_batch_g2_poly_eval_device(bn254_ctx *ctx, const uint8_t *d_coeffs, const uint64_t *d_poly_off, size_t p, const uint32_t *d_eval_poly,
                                    const uint32_t *d_eval_x, size_t q, uint8_t *d_out, uint8_t *d_status, void *stream);
/* REGISTER THE SHARE KEYS OF A COMMITMENT VECTOR: pk_j = f(j + 1) G2 = sum over k < t of (j + 1)^k C_k for j < n_keys, from the t
 * commitments (host memory, uncompressed).  The evaluation's output stays in device memory and is read where it lies by the kernel every
 * registration runs; only key_status and one status byte come home.
 * DEFINING IDENTITY: the context afterwards is indistinguishable from bn254_ctx_register_keys on the n_keys outputs of
 * bn254_batch_g2_poly_eval at x = 1 .. n_keys with the same flags; registration's own subgroup check still judges every key.  Like every
 * registration it quiesces the context and drops the previous key set and the group key first.  If a commitment does not decode, *status is
 * that decode status (the lowest index wins), NO keys are registered (the context then has none) and key_status is untouched; otherwise
 * *status = 0.  BN254_E_BAD_ARGUMENT: t == 0, n_keys == 0, n_keys >= 2^32, NULL commitments or status.  The call does NOT install the group
 * key: the caller names C_0 with bn254_ctx_set_group_key, which applies its own checks.  A key set registered this way passes
 * bn254_ctx_check_dealing at threshold t by construction. */
int bn254_ctx_register_keys_commitments(bn254_ctx *ctx, const uint8_t *commitments /* t*128, host */, uint32_t t, size_t n_keys, uint32_t flags,
                                        uint8_t *key_status /* n_keys, or NULL */, uint8_t *status /* 1 */);

/* COMBINE VECTORS OF G2 POINTS, one scalar per vector, column by column: d vectors of len points each (vector-major: point k of vector i
 * is entry i*len + k), d scalars of 32 big-endian bytes:  out[k] = sum over i of scalars[i] * vectors[i][k].  What a linear combination of
 * commitment vectors is — of the sub-dealings of a reshare (below), of the dealers of a DKG under weights.
 * DEFINING IDENTITY: out[k] and status[k] are byte for byte bn254_batch_g2_msm over ONE segment holding vectors[0][k], .., vectors[d-1][k]
 * with the scalars 0 .. d-1 and the same reduce_scalar.  So: points are decoded with flags 0 (on the curve, NO subgroup check); the first
 * non-zero decode status in vector order wins and the output is then 128 zero bytes; a fault in one column touches that column only; d = 0
 * gives identities with status 0; scalars >= r are reduced (reduce_scalar != 0) or taken as they are, as there.
 * Arguments: len = 0 returns 0 and writes nothing; d*len >= 2^32 is BN254_E_BAD_ARGUMENT; otherwise the argument, alignment and NULL rules of
 * bn254_batch_g2_msm_device (vectors, scalars and out 4-byte aligned in the _device form, else BN254_E_MISALIGNED; vectors and scalars may be
 * NULL only when d = 0).  Both sizes are arguments, so the _device form copies nothing home: it only enqueues.  One call per context in
 * flight.  Scratch: 363 B per term (146 B per decoded point, the 216-byte term and its status byte).
 * Cost: every point is decoded ONCE; one lane per term walks the 256-step ladder over the decoded limbs, in column-major term order (with
 * d >= 64 a wave holds 64 consecutive vectors of one column: its point loads are strided by len points — one load beside 256 ladder
 * steps); then the two segment sums of bn254_batch_g2_msm, split by BN254_OPT_COLLECT_WAVE_MIN_SHARES over d.
 * Which call when: this one where the scalars belong to the vectors — it stages d scalars and no transposed copy, where bn254_batch_g2_msm
 * takes d*len of each; bn254_batch_g2_msm for a scalar per point.  Measured: under bn254_ctx_reshare_commitments below (a tie to a slight win
 * against bn254_batch_g2_msm with its inputs staged; the transposed copy and the replicated scalars are what is saved).
 * Out of scope: the multi-GPU layer, compressed points, a G1 form, a bucket or bit-sliced sum for thousands of vectors, slicing. */
int bn254_batch_g2_vector_combine(bn254_ctx *ctx, const uint8_t *vectors /* d*len*128, vector-major */, const uint8_t *scalars /* d*32 */,
                                  size_t d, size_t len, int reduce_scalar, uint8_t *out /* len*128 */, uint8_t *status /* len */);
int bn254_batch_g2_vector_combine_device(bn254_ctx *ctx, const uint8_t *d_vectors, const uint8_t *d_scalars, size_t d, size_t len,
                                         int reduce_scalar, uint8_t *d_out, uint8_t *d_status, void *stream);
/* RESHARE A THRESHOLD KEY: the commitments of the NEXT committee's polynomial from the sub-dealings of the old members.  Old member i —
 * registered key dealer_key[i] — deals its share s_i with a polynomial g_i of degree t_new - 1, g_i(0) = s_i, and publishes the t_new
 * commitments D_i (vectors, dealer-major, host memory, uncompressed); D_i,0 must be its registered key.  For a set S of `threshold`
 * qualified dealers f' = sum lambda_i(S) g_i has f'(0) = f(0): commitments[k] = sum over i in S of lambda_i(S) D_i,k, and the group key stays.
 * The registered set is the OLD committee; the call reads it and leaves the context as it found it.  Host-synchronous; quiesces first, like
 * bn254_ctx_check_dealing.
 * BN254_E_BAD_ARGUMENT: a NULL argument; d = 0, t_new = 0 or threshold = 0; flags != 0; no registered keys; bm_words < ceil(n_keys / 32);
 * dealer_key not STRICTLY INCREASING (checked on the host: all parties must agree on the order, and two vectors of one dealer are an
 * equivocation for the protocol to settle, not for this call); d*t_new >= 2^32.
 * dealer_status[i] is the FIRST that applies: (1) dealer_key[i] >= n_keys: 2; (2) the key's registration status is non-zero: that status — a
 * failed proof of possession counts, as in every keyed call; (3) a commitment of the vector does not decode (flags 0): the first non-zero
 * status in coefficient order; (4) D_i,0 is not the registered key as a group element: 9 — field elements are compared, so a registered
 * identity key needs 128 zero bytes and the negated key (same x, -y) reads 9; (5) else 0.  With Q the dealers of status 0:
 *   |Q| >= threshold: S = the `threshold` lowest key indices of Q — a choice that depends on nothing but Q —, used_bits = S in the bitmap
 *     calls' numbering (exactly `threshold` bits), commitments as above with lambda the coefficient of bn254_batch_threshold_combine_keyed
 *     (x_j = j + 1), *status = 0;
 *   |Q| < threshold (threshold > n_keys and threshold > d included): *status = 9, commitments are zero bytes, used_bits = Q.
 * Words of used_bits past the last key are zero.
 * DEFINING IDENTITY 1: on success commitments is byte for byte bn254_batch_g2_vector_combine of S's vectors in increasing key order with the
 * scalars bn254_debug_lagrange_at_zero gives for x = key + 1 and reduce_scalar = 0.
 * DEFINING IDENTITY 2 (closed loop): over registered keys that are an honest threshold-of-n dealing, and honest sub-dealings, commitments[0]
 * is the group key bn254_ctx_check_dealing(threshold) returns, whatever S; registered with bn254_ctx_register_keys_commitments, the keys of
 * `commitments` pass bn254_ctx_check_dealing(t_new) with that same key.
 * NOT checked: that the registered keys are a dealing — bn254_ctx_check_dealing's job, once per set; that the private sub-shares match the
 * vectors — each recipient's share check against the dealer's vector (secret * G2 == the vector at index + 1, bn254_batch_g2_poly_eval), whose
 * complaints decide which dealers the caller passes in.
 * Cost: every commitment is decoded once; a lane per dealer settles its status, one wave ranks the qualified ones, a lane per taken dealer
 * computes its coefficient in Fr; then threshold * t_new ladders — untaken dealers cost none — and the sums.  One wait brings
 * dealer_status, the row, the commitments and the status home.  Scratch: 146 B per commitment given, 217 B per term.
 * Measured on an MI355X (tools/reshare_throughput.py, profiles/reshare.jsonl; whole calls under a host clock, staging on both sides, median
 * [min, max] of 7 alternating runs after 2 warm-up runs; every old member a dealer, (n, t) -> (n, t); the baseline is the route that exists
 * without the calls and checks nothing about the dealers: the coefficients of S in Python integers, the vectors of S transposed and the
 * scalars replicated t times in Python, bn254_batch_g2_msm over t segments of t terms, each part timed).  (256, 171): this call 7.23 ms
 * [7.03, 7.25] against 5.08 [5.06, 5.15] + 4.68 [4.13, 4.94] + 6.21 [6.18, 6.24]; bn254_batch_g2_vector_combine on the 171 vectors of S 6.16
 * [6.15, 6.16].  (1 024, 683): this call 63.8 [54.8, 74.4] against 72.6 [72.5, 74.0] + 87.1 [86.1, 94.8] + 53.8 [52.5, 56.2]; the vector
 * combine 52.4 [52.3, 52.5].  The call's own part is about 10 ms MORE than bn254_batch_g2_msm alone at (1 024, 683), outside the spreads:
 * it stages and decodes the vectors of all 1 024 dealers (89 MB) to qualify them, where the old route is handed the 683 of S; it wins by the
 * host's coefficients and staging.  bn254_batch_g2_vector_combine against bn254_batch_g2_msm with everything staged for it: 6.16 against
 * 6.21 and 52.4 against 53.8 — a tie to a slight win; what it saves is the transposed copy and the replicated scalars.  The same bytes on
 * all three routes.  bn254_batch_g2_msm (171 terms), bn254_ctx_check_dealing (256, 171) and bn254_batch_g2_poly_eval (256, 171) in this
 * build against the parent's, two alternating runs each: 5.34 / 5.35 against 5.34 / 5.36, 7.07 / 7.08 against 7.10 / 7.09, 6.09 / 6.09
 * against 6.09 / 6.08 ms — within each other's spreads, the same output bytes.
 * Unmeasured: other thresholds and t_new != threshold, fewer dealers than members, more than 1 024 keys, disqualified dealers at scale, the
 * _device form of the vector combine under events, a sweep of the lane/wave split of the sums for this call.
 * Which call when: this one for the reshare itself; bn254_batch_g2_vector_combine where the caller has its own qualification rules or its
 * own scalars — and, for committees of a thousand, where the caller knows S already and would rather not stage the vectors outside it.
 * Out of scope: a _device form, compressed commitments, the multi-GPU layer, a bucket or bit-sliced sum for committees of
 * thousands (the cost here is threshold * t_new ladders), slicing, the reshare protocol's rounds and complaints. */
int bn254_ctx_reshare_commitments(bn254_ctx *ctx, const uint8_t *vectors /* d*t_new*128, host, dealer-major */,
                                  const uint32_t *dealer_key /* d, host, strictly increasing */, size_t d, uint32_t t_new,
                                  uint32_t threshold /* the OLD committee's t */, uint32_t flags /* must be 0 */,
                                  uint8_t *dealer_status /* d */, uint32_t *used_bits /* bm_words */, size_t bm_words,
                                  uint8_t *commitments /* t_new*128 */, uint8_t *status /* 1 */);

/* OPTIMISTIC THRESHOLD COMBINE: interpolate first, verify the result once per tuple under the group key.  The interpolated signature is
 * unique: if it verifies under f(0) * G2::one() it is THE group signature whatever the individual shares were, so one pairing check per
 * tuple proves the output — and proves exactly what the consumer will check.  (The optimistic collect's check of the plain sum cannot be
 * reused: errors that cancel in the sum of the shares do not cancel under the coefficients.)
 * Arguments, argument checks, alignment rules, the range rule, the fill of share_status with 2, BN254_OPT_MAX_CHUNK slicing (tuples in pieces
 * for hash and tuple check, shares in pieces for the queue), bn254_ctx_expect_msgs_len and threshold == 0 are exactly those of
 * bn254_batch_threshold_combine_keyed[_device]; in addition a context with no group key set returns BN254_E_BAD_ARGUMENT.  The _device form only
 * enqueues, on the caller's stream, and never synchronises with the host; one call may be in flight per context.
 * Per accepted tuple i (range rule passed, hash status 0; a refused tuple gets the exact call's bytes):
 *   1. every share gets the checks short of the pairing (decode, key index, registration status: rules 1-3 of the optimistic collect); a
 *      share whose status is 0 is a CANDIDATE; C_i = the keys with a candidate.
 *   2. a tuple in which a key has two candidates, or with |C_i| < threshold, goes the exact way at once.
 *   3. else S'_i = the `threshold` lowest keys of C_i, and the group signature is sum over j in S'_i of lambda_j(S'_i) sigma_j, by the exact
 *      call's coefficient, term and sum kernels under a mask.
 *   4. the tuple check: e(H(m_i), GPK) * e(group_sig_i, -G2) == 1, the signature decoded with flags 0 (the identity is legitimate), by the
 *      keyed verify's routing (lane machine, expanded key on the small-batch kernels, or lane pairs on the group key's line table).
 *   5. PASS: tuple_status 0 and group_sigs[i] as computed, used_bits row = S'_i, n_valid[i] = |C_i|, the share statuses the pre-check's.
 *   6. FAIL, or flagged in 2: the tuple's candidates are verified one by one on the device through a queue, its row is rebuilt from the
 *      verified statuses, and rank-and-select, the coefficients and the weighted sum run again for these tuples only (a gate masks the
 *      others; a wave with nothing to take leaves at once).  All five outputs of such a tuple are byte for byte the exact call's.
 * Everything is enqueued whether or not a tuple fails: the host never learns.  No seed, no randomness.
 * WHAT IS PROVED: for a tuple with tuple_status 0, bn254_batch_verify of (m_i, group_sigs[i], GPK) returns 0 — the tuple check proved it, or
 *   the tuple went the exact way and the exact call's own guarantee applies.
 * IDENTITY A: whenever every share of S'_i is individually valid, tuple_status, group_sigs and the used_bits row equal the exact call's (then
 *   V contains S' and lies in C, so the lowest t of V are S').
 * IDENTITY B: a tuple that goes the exact way equals the exact call in all five outputs.
 * DEVIATION 1: in a passing tuple the shares outside S'_i were not verified: they read their pre-check status and n_valid counts candidates.
 *   A caller who needs per-share verdicts takes the exact call.
 * DEVIATION 2: shares of S'_i whose errors cancel under the coefficients (sigma_a + lambda_b D and sigma_b - lambda_a D) read 0 in a passing
 *   tuple; the group signature is still the valid one.  The exact call would have dropped both keys.
 * WHOLE-CALL ROUTING: the call IS the exact call (same bytes, by identity B) when n_shares < BN254_OPT_THRESHOLD_OPT_MIN_SHARES, when no keys
 *   are registered, or with BN254_OPT_PAIR_LANES = 0.
 * Under bn254_ctx_set_profiling: ms[0] front end and candidate rows, ms[1] coefficients and weighted sum, ms[2] the tuples' Miller loop and
 * final exponentiation, ms[3] exact fallback and re-interpolation (a call in several pieces: the last piece's ms[1] boundary).
 * Measured on an MI355X (tools/threshold_throughput.py --optimistic, profiles/threshold_optimistic.jsonl; 256 dealt keys, threshold = two
 * thirds of a tuple's keys, the true group key set; _device forms under HIP events, the two calls alternating in one process, median [min,
 * max] of 7; optimistic against exact, ms).  Every share valid: 256 tuples x 171 shares 4.46 [4.43, 4.49] against 11.50 [11.45, 11.59];
 * 1 024 x 171 11.38 [11.32, 11.40] against 34.59 [34.45, 34.70]; 2 048 x 171 20.33 [20.16, 20.40] against 62.67 [62.39, 63.15]; 4 096 x 11 5.53
 * [5.49, 5.55] against 11.29 [11.19, 11.44]; 64 x 171 3.84 against 7.49; 36 x 171 3.84 against 5.32; 18 x 171 3.85 against 5.22; 9 x 171 3.87
 * [3.82, 4.06] against 4.73 [4.68, 4.83]; 3 x 171 3.81 [3.78, 4.00] against 4.03 [3.97, 4.12].  Stages of one profiled call at 256 x 171: front
 * end 0.20, coefficients and weighted sum 3.22, tuple check 0.94, fallback 0.10; at 2 048 x 171: 0.26, 18.11, 1.66, 0.16 — the weighted sum
 * (a 128-step ladder per kept share) is what is left, and it grows with the shares where the exact call's pairings grow three times as fast.
 * When something fails: ONE failing tuple costs the call one pass of the queue's lane-pair kernels, about 7.4 ms whatever the queue's length —
 * 256 x 171 11.76 [11.74, 11.87] against 12.14 [12.03, 12.18], 2 048 x 171 27.59 [27.46, 28.24] against 64.03 [63.74, 64.50]; 1 % wrong shares
 * at 1 024 x 171 (708 of 1 024 tuples go exact) 37.12 [36.85, 37.63] against 34.74 [34.59, 35.12]: it LOSES; the WRONG group key at 256 x 171
 * (every tuple goes exact: the cost of a misconfiguration) 15.53 [15.46, 15.59] against 11.52 [11.39, 11.59]; one tuple of 4 096 shares over
 * 256 keys (every key several times: a duplicate, exact at once) 9.53 [9.39, 9.62] against 6.27 [6.14, 6.38]: it LOSES.  So: this call when
 * shares are almost all valid and a tuple names each key once; the exact call when many tuples hold a bad share among their lowest keys, when
 * tuples repeat keys, or when per-share verdicts matter.  Unmeasured: calls below 513 shares, other thresholds, more than 256 keys, the host form.
 * DESIGN.md section 10l. */
int bn254_batch_threshold_combine_keyed_optimistic(bn254_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */,
                                                   const uint8_t *shares /* n_shares*64 */, const uint32_t *share_key /* n_shares */,
                                                   const uint64_t *share_off /* n+1 */, size_t n_shares, size_t n, size_t bm_words,
                                                   uint32_t threshold, uint32_t flags, uint8_t *share_status /* n_shares */,
                                                   uint8_t *tuple_status /* n */, uint8_t *group_sigs /* n*64 */,
                                                   uint32_t *used_bits /* n*bm_words */, uint32_t *n_valid /* n, or NULL */);
int bn254_batch_threshold_combine_keyed_optimistic_device(bn254_ctx *ctx, const uint8_t *d_msgs, const uint64_t *d_msg_off, const uint8_t *d_shares,
                                                          const uint32_t *d_share_key, const uint64_t *d_share_off, size_t n_shares, size_t n,
                                                          size_t bm_words, uint32_t threshold, uint32_t flags, uint8_t *d_share_status,
                                                          uint8_t *d_tuple_status, uint8_t *d_group_sigs, uint32_t *d_used_bits,
                                                          uint32_t *d_n_valid, void *stream);

/* compressed wire formats (src/utils.rs:84-104, :130-158): out = uncompressed point, status as
 * bn::G1::from_compressed / bn::G2::from_compressed report through src/types.rs:91-93, :233-237, checked in the order
 * those decoders work (an input with several faults reports the first):
 *   G1: x >= q -> 6 NotMemberError; no square root -> 6; prefix byte not 0x02 / 0x03 -> 3 InvalidEncoding.
 *   G2: x.im >= q (the U512 does not split into two field elements) -> 6 NotMemberError; no square root -> 6; sign
 *       byte not 0x0a / 0x0b -> 3; not in the order-r subgroup -> 6.
 * (The x.im >= q code is UNPINNED: no reference vector exists and zeropool-bn is not vendored.  Upstream's
 * Fq2::from_slice is recalled as mapping a missing `divrem` quotient through `ok_or(FieldError::NotMember)`, which
 * src/error.rs:44-51 turns into NotMemberError; library versions before 0.6 returned 3 here.) */
int bn254_batch_g1_decompress(bn254_ctx *ctx, const uint8_t *in /* n*33 */, size_t n, uint8_t *out /* n*64 */, uint8_t *status);
int bn254_batch_g2_decompress(bn254_ctx *ctx, const uint8_t *in /* n*65 */, size_t n, uint8_t *out /* n*128 */, uint8_t *status);
/* The _device form of bn254_batch_g1_decompress: the same bytes (a failed item: its status and 64 zero bytes), device pointers, only
 * enqueues.  d_in33 needs no alignment, d_out64 is 4-byte aligned (else BN254_E_MISALIGNED); n < 2^32; n == 0 returns 0.  A caller that
 * goes on into a registered-key call does not need it: BN254_FLAG_G1_COMPRESSED decompresses inside the call and keeps the statuses apart
 * (a failed item's 64 zero bytes here are the identity, which decodes). */
int bn254_batch_g1_decompress_device(bn254_ctx *ctx, const uint8_t *d_in33 /* n*33 */, size_t n, uint8_t *d_out64 /* n*64 */,
                                     uint8_t *d_status /* n */, void *stream);

/* timing of the most recent batch_verify*(…) on this context, from HIP events recorded on the
 * launch stream around each kernel: ms[0] decode, ms[1] hash-to-G1, ms[2] Miller loop,
 * ms[3] final exponentiation.  Synchronises the stream.  Requires bn254_ctx_set_profiling(ctx, 1). */
int bn254_ctx_set_profiling(bn254_ctx *ctx, int enabled);
/* Options a CALLER may want to touch: the batch-size thresholds of the routing table (which kernel layout serves which batch size — ONE
 * table, bn254_amd/csrc/bn254_ws.h: bn_route; defaults measured on an MI355X), the thresholds of the aggregate / randomised paths, and the
 * staging mode of the host-pointer verify.  Every setting returns the same status bytes; they trade latency against throughput.
 * (The A/B layouts of earlier rounds — one lane per verify, one pairing per lane, four wave roles, lane groups — and the test / measurement
 * knobs are developer options: section BN254_DEV_HOOKS at the end of this header.) */
#define BN254_OPT_TRIO_MAX_BATCH 6 /* verify / check_public_keys batches of up to this many items run in the OCTET layout (eight lanes per item: the
                                     three Fq6 products of every Fq12 operation in three lane pairs) — fewer instructions per lane, i.e. lower
                                     latency when the batch cannot fill the chip anyway; same status bytes.  Default 16384 (two passes of one wave
                                     on each of the 1024 SIMDs: 2.3 ms for 1 verify, 3.3 ms for 8192, 6.3 ms for 16384, against 6.4 / 7.1 /
                                     7.9 ms on lane pairs); 0 = never */
#define BN254_OPT_NONET_MAX_BATCH 13 /* small batches: up to this many items the final exponentiation runs on NINE lane pairs per item (18 lanes,
                                      three items per wave): the nine squarings of a cyclotomic squaring at once, the 18 products of an Fq12
                                      multiplication in two rounds; same status bytes.  0 = never (octet layout) */
#define BN254_OPT_LM_MAX_BATCH 15 /* small batches: up to this many items the Miller loop runs as the LANE MACHINE (nine lane pairs in each of four
                                   waves per item: every product of a dependency level in its own lane pair; twist-point formulas rearranged
                                   for depth; bn254_batch_verify_keyed: its keyed form on the registered keys' line tables); same status
                                   bytes.  0 = never (wave roles / octet layout) */
#define BN254_OPT_RAND_MIN_BATCH 5 /* randomised verify: batches with fewer items run the exact kernels instead (same statuses; group_ok = no item of the
                                     group failed the pairing check).  Default 131072, the measured break-even on an MI355X; 0 = always randomised */
#define BN254_OPT_AGG_RAND_MIN_PAIRS 26 /* bn254_batch_aggregate_verify_distinct_keyed_randomized: calls with fewer messages take the exact keyed route
                                         (same statuses).  Default 65536, the measured break-even on an MI355X; 0 = always randomised */
#define BN254_OPT_AGG_SUBSET_MIN_TUPLES 9 /* aggregate verify: from this many tuples on (default 4096) the sums of all subsets of every 8 consecutive
                                            keys of the pool are tabulated once per call and a tuple adds one table entry per group instead of one
                                            key per signer (pools of up to 2048 signers, lists longer than n_signers / 8); 0 = never.  Same statuses. */
#define BN254_OPT_AGG_WIDE_MIN_TUPLES 14 /* aggregate verify: from this many tuples on (default 262144) the subset-sum tables are WIDENED once more —
                                          keys: the sums of all subsets of every 16 consecutive signers (n_signers / 16 x 65536 entries, 671 MB
                                          for 1024 signers), signatures per message: of every 8 — by one batched affine addition per entry, so
                                          that a tuple adds half as many entries; 0 = never.  Same statuses. */
#define BN254_OPT_PINNED_STAGING 12 /* bn254_batch_verify (host pointers), batches of >= 8192: T = 1..16 threads copy the caller's (pageable)
                                     buffers through a pinned staging buffer of the context in 1 MB pieces, each piece's DMA enqueued as soon
                                     as it is in place; 0 = hipMemcpyAsync straight from the caller's buffers (the runtime stages them) */
#define BN254_OPT_MAX_CHUNK 17 /* *_device and host entry points of verify / verify_compressed / verify_keyed: a batch of more than this many items
                                is processed in slices of this size (the 792 B/item workspace of a slice is reused; statuses land at the items'
                                own positions, so the result is that of one call).  0 (default) = automatic: slice only when the workspace of
                                the whole batch does not fit the device's free memory */
#define BN254_OPT_KEY_DEDUP 20 /* bn254_batch_verify_device on lane pairs (batches above the small-batch family): 1 (default) = find the batch's distinct
                                public keys on the device and tabulate each one's 87 Miller-loop lines once per call (the format of
                                bn254_ctx_register_keys), beside the decode and hash kernels on a stream of the context; the Miller loop then reads
                                the tables (k_miller_verify_keyed_pair) when the thresholds below hold, decided on the device without a host sync.
                                0 = always the generic loop.  Same status bytes either way */
#define BN254_OPT_KEY_DEDUP_MAX_KEYS 21 /* ... tables for at most this many distinct keys per call (default 1024; 20.6 KB of device memory each) */
#define BN254_OPT_KEY_DEDUP_MIN_MULT 22 /* ... and only when the batch has at least this many items per distinct key (default 16) */
#define BN254_OPT_KEY_CACHE 36 /* ... 1 (default) = the line tables stay in the context between calls, found again by the key's 128 bytes (the
                                context keeps its own copy; the caller's buffer may be freed or rewritten): a call builds only the keys no
                                earlier call has built, and a service with a stable key set builds none from its second call on.  Held within
                                the memory of BN254_OPT_KEY_DEDUP_MAX_KEYS rows; when a call's new keys do not fit the free rows the cache
                                is dropped and the call builds all its keys.  Also dropped: by other decode flags than the last call's, a
                                change of the KEY_DEDUP options above, a growth of the dedup buffers, and by setting this option (0 = every
                                call builds all its keys).  A call that takes the generic loop leaves it as it was; a key with a degenerate
                                line is never kept.  ORDERING: the cache is written on a stream of the context during one call and read by
                                the next.  A call of this route therefore waits ON THE DEVICE, through an event the context owns, for the end
                                of the previous call of this route before it touches the dedup buffers — also when the two are enqueued on
                                different caller streams with no host synchronisation in between.  (The rule above for everything else a
                                context shares stands: one call in flight.)  Same status bytes, same table words */
#define BN254_OPT_BITMAP_TABLE_MAX_KEYS 28 /* bn254_batch_verify_keyed_bitmap: subset tables of the registered set while it has at most this many keys
                                             (default 4096: 5 152 B per key, 21 MB); above, or with 0, the selected keys are added one by one.
                                             Same status bytes */
#define BN254_OPT_BITMAP_RAND_MIN_TUPLES 33 /* bn254_batch_verify_keyed_bitmap_randomized: calls (slices) with fewer tuples take the exact bitmap call
                                             (same statuses).  Default 81920, the smallest measured size from which the 128-bit variant wins at
                                             256 keys; 0 = always randomised */
#define BN254_OPT_BITMAP_RAND_MAX_KEYS 35 /* ... and when more keys than this are registered (same statuses): the G1 side costs one addition per
                                           bitmap byte and tuple, which at 1 024 keys outweighs what the route saves at every size measured.
                                           Default 256 */
#define BN254_OPT_COLLECT_WAVE_MIN_SHARES 37 /* bn254_batch_collect_keyed_bitmap, developer option: tuples with at least this many shares are summed by
                                               one wave each (64 partial sums and a tree), shorter ones by one lane each; >= 1.  Default 16 — a
                                               figure NOBODY HAS MEASURED beyond three shapes (tools/collect_throughput.py --wave-min: tuples of 11 shares sum in 0.18 ms by lanes
                                               against 0.62 by waves, tuples of 171 in 0.24 by waves against 1.86 by lanes; nothing in between).  Same bytes either way */
#define BN254_OPT_COLLECT_RAND_MIN_SHARES 38 /* bn254_batch_collect_keyed_bitmap_randomized: calls with fewer shares take the exact collect (same
                                               bytes).  Default 65664, the smallest measured size from which the call wins over 256 keys
                                               (at 45 056 shares it ties or loses; nothing measured in between); 0 = no lower bound */
#define BN254_OPT_COLLECT_RAND_MIN_PER_KEY 39 /* ... and calls with fewer than this many shares per registered key (n_shares / n_keys, rounded
                                                down): groups are per key, so few shares per key mean padded groups.  Default 42, the smallest measured
                                                ratio at which the call wins (175 104 shares over 4 096 keys; at 10 per key it loses;
                                                nothing measured in between); 0 = no lower bound */
#define BN254_OPT_COLLECT_OPT_MIN_SHARES 40 /* bn254_batch_collect_keyed_bitmap_optimistic: calls with fewer shares take the exact collect (same
                                              bytes).  Default 1539, the smallest measured size from which the call wins with every share
                                              valid (tuples of 171 shares over 256 keys: 1.86 ms against 2.09; at 1 026 shares it ties, at 513
                                              it loses; nothing measured in between).  Calls made of one- or two-share tuples lose at every
                                              size measured, which a count of shares cannot see; 0 = no lower bound */
#define BN254_OPT_COLLECT_OPT_MIN_TUPLE_SHARES 41 /* ... and, per tuple, tuples with fewer candidates go the exact way.  Default 1: every tuple
                                                    with a candidate is checked.  Measured: a tuple sent the exact way costs the call one pass
                                                    of the queue's kernels, 4.9 ms whatever the queue's length, while the check of a short
                                                    tuple's sum adds nothing measurable to the pass over the other tuples — so no measured
                                                    size favours a higher value (calls of ONLY one- or two-share tuples lose 0.8 ms to the
                                                    exact call as a whole; tuples of four win).  The option stays for callers who want short
                                                    tuples verified share by share; 0 and 1 mean the same */
#define BN254_OPT_MERGE_WAVE_MIN_PARTS 43 /* bn254_batch_merge_keyed_bitmap, developer option: tuples with at least this many partials are merged by
                                            one wave each (select parallel in the words of the row, 64 partial sums and a tree), shorter
                                            ones by one lane each; >= 1.  Default 16, from the sweep of tools/merge_throughput.py --sweep
                                            (select-and-sum ms, lane / wave, 16 384 partials per call): rows of 8 words — 8 partials 0.15 /
                                            0.41, 16 0.25 / 0.40, 32 0.44 / 0.30, 64 0.82 / 0.24, 256 3.10 / 0.36; rows of 128 words — 4 0.26
                                            / 0.63, 8 0.45 / 0.42, 16 0.84 / 0.42, 32 1.60 / 0.32, 256 12.4 / 0.49.  The crossing lies
                                            between 16 and 32 partials at 8 words and at 8 at 128 words; 16 loses 0.15 ms at (8 words, 16
                                            partials) where 32 would lose 0.42 ms at (128 words, 16 partials).  Lengths between the
                                            powers of two were not measured.  Same bytes either way */
#define BN254_OPT_MERGE_OPT_MIN_PARTS 45 /* bn254_batch_merge_keyed_bitmap_optimistic: calls with fewer partials take the exact merge (same
                                           bytes).  Default 64, the smallest measured size from which the call wins beyond the spread with every partial
                                           valid (tuples of 16 partials over 256 keys: 4 x 16 1.81 ms against 1.86; 2 x 16 and 1 x 16 tie;
                                           nothing measured between 32 and 64 partials).  A call whose tuples hold overlapping candidates
                                           loses at any size, which a count of partials cannot see; 0 = no lower bound */
#define BN254_OPT_THRESHOLD_OPT_MIN_SHARES 46 /* bn254_batch_threshold_combine_keyed_optimistic: calls with fewer shares take the exact call (same
                                                bytes).  Default 513, the smallest measured size (3 tuples x 171 shares over 256 keys, every share valid: 3.81 ms
                                                [3.78, 4.00] against 4.03 [3.97, 4.12] — it wins by more than the exact call's own spread); no
                                                measured size loses with every share valid, and nothing below 513 shares was measured, so
                                                smaller calls take the exact call; 0 = no lower bound */
#define BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS 0 /* (number 0: 1 to 46 are taken and tests/test_threshold_optimistic.py pins 46 as the highest)
                                                  bn254_batch_g2_poly_eval, bn254_ctx_register_keys_commitments: polynomials with at least this many
                                                  coefficients are evaluated by a wave each, shorter ones by a lane each (same bytes
                                                  either way; 1 = always a wave, a large value = always a lane).  Default 16, swept (tools/poly_eval_throughput.py --sweep, profiles/poly_eval.jsonl;
                                                  256 evaluations of one polynomial, host form, median of 7): 8 coefficients 2.63 ms in lanes against
                                                  5.45 in waves; 16 coefficients 5.44 against 5.45 at a 9-bit x (a tie) and 6.06 [6.04, 6.07]
                                                  against 5.46 [5.45, 5.46] at a 13-bit x; 32: 11.1 / 12.4 against 5.45 / 5.47; 64: 22.4 / 25.0
                                                  against 5.45 — 16 is the smallest swept length at which the wave layout wins beyond the
                                                  spread; nothing between 8 and 16 was measured */
int bn254_ctx_set_option(bn254_ctx *ctx, int option, int value);
/* per-kernel times of the last verify-shaped call with profiling on (HIP events on the call's stream):
 * ms[0] decode, ms[1] hash-to-G1, ms[2] Miller loop, ms[3] final exponentiation.  The host-pointer bn254_batch_verify runs
 * the hash first and its ms[1] includes the transfer of the messages.  Other *_device calls reuse the slots: pairing ms[1] = 0;
 * hash_to_g1 ms[0] = the filter rounds (SHA-256 + Jacobi symbol per tested counter), ms[1] = the square roots (one per message), ms[2] = encoding the
 * points, ms[3] = 0; aggregate_verify ms[0] = the pools
 * (decoding, hashing the messages, the subset-sum table), ms[1] = the aggregation kernel; verify_keyed_bitmap ms[0] = sigma's decode + hash-to-G1,
 * ms[1] = the aggregate keys (the summation kernel; the lazy table build runs ahead of ms[0]), ms[2] Miller loop, ms[3] final exponentiation;
 * collect_keyed_bitmap ms[0] = decode + hash-to-G1 (once per tuple) + spread, ms[1] = select-and-sum (it runs last), ms[2] Miller loop,
 * ms[3] final exponentiation (the last slice's; the hash counts in ms[0] only when the call ran in one piece);
 * collect_keyed_bitmap_randomized on its randomised route the same four with ms[2] = grouping by key + scalar ladders, ms[3] = group checks +
 * exact re-checks of failed groups;
 * collect_keyed_bitmap_optimistic on its optimistic route ms[0] = front end (hash, range rule, pre-check) + provisional sum, ms[1] = the
 * aggregate keys, ms[2] = the tuples' Miller loop and final exponentiation, ms[3] = exact fallback + re-sum (a call whose tuples are checked
 * in several pieces: ms[1] runs from the provisional sum to the last piece's keys);
 * merge_keyed_bitmap the exact collect's four: ms[0] = front end (hash-to-G1 once per tuple, decode, spread, aggregate keys), ms[1] =
 * select-and-sum (it runs last), ms[2] Miller loop, ms[3] final exponentiation (the last slice's);
 * merge_keyed_bitmap_optimistic on its optimistic route ms[0] = front end (hash, range rule, pre-check) + provisional select-and-sum, ms[1] =
 * the aggregate keys of the union rows, ms[2] = the tuples' Miller loop and final exponentiation, ms[3] = fallback + re-select (a call whose
 * tuples are checked in several pieces: ms[1] runs from the provisional select to the last piece's keys). */
int bn254_ctx_last_kernel_ms(bn254_ctx *ctx, float ms[4]);
/* with BN254_OPT_CLOCK_PROBE on: achieved shader clock in MHz of the lane-pair Miller kernels [0], final exponentiations [1] and probe
 * kernels (bn254_probe_issue_rate, bn254_probe_leaf_floor) [2] launched on this context SINCE THE PREVIOUS CALL of this function (or
 * since the option was set) — the counters accumulate over launches and every call reads and clears them, so a caller brackets exactly
 * the launches it wants the clock of (bench.py: the timed steps).  0 = no such kernel ran in between.  Synchronises the device. */
int bn254_ctx_last_clocks(bn254_ctx *ctx, double sclk_mhz[3]);

/* =====================================================================================================================
 * Multi-GPU: the batch sharded over the GPUs of one node, ONE process (bn254_mgpu.hip).
 *
 * Every tuple of a batch is independent (/root/reference/src/ecdsa.rs:49-64 shares no state between calls), so a batch of n
 * items splits into G contiguous shards of S = ceil(n / G) items (the last ones shorter or empty): shard g = items
 * [g*S, min((g+1)*S, n)).  A bn254_mgpu owns, per entry of `devices`, one bn254_ctx, one stream and one host worker thread
 * (started once at creation; no thread is created per call, nothing is ever exec'ed).  The ONLY exchange between devices is
 * the gather of the per-item status bytes (and, for the pairing entry point, an 8-byte sum): RCCL's C API over xGMI
 * (ncclAllGather / ncclAllReduce on ncclCommInitAll communicators; librccl.so.1 is loaded with dlopen at the first call that
 * needs it, so single-GPU users of the library never load it).  A device may be listed more than once — several contexts on
 * one GPU, which is how the single-GPU test rigs run this code; RCCL refuses two ranks on one device, so such a handle gathers
 * with peer copies (hipMemcpyPeerAsync, pulled by every destination on its own stream) instead; BN254_MGPU_OPT_GATHER selects
 * either explicitly.  This is the layer /root/reference/src/lib.rs:60-63 would grow an `ECDSA::batch_verify(&Gpus, ...)` on
 * (INTEGRATION.md).
 *
 * Host-pointer entry points (bn254_mgpu_batch_verify, _batch_pairing, _batch_hash_to_g1): the caller passes the WHOLE batch;
 * every worker stages its shard to its device, runs the single-GPU entry point of the same name and copies the results straight
 * into the caller's slices — no collective.  They return when all shards are done; the return value is the first non-zero
 * return code of any shard (all shards are always run to the end).
 *
 * *_device entry points: the caller passes, per device g, DEVICE pointers to shard g's inputs (resident on devices[g], offsets
 * relative to that shard's own message buffer) and a status buffer d_status_all[g] of bn254_mgpu_gathered_len(mg, n) = G*S
 * bytes; device g writes its shard's statuses at offset g*S of ITS buffer and the gather (in place) leaves every device with
 * all n status bytes at d_status_all[g][0 .. n).  streams[g] (hipStream_t as void*; the array or an entry may be NULL = the
 * handle's own stream of that device) carries the kernels and the collective of device g; the calls only enqueue.
 * A handle carries one call in flight, like a context. */
typedef struct bn254_mgpu bn254_mgpu;

int bn254_mgpu_create(const int *devices, int n_dev /* 1..64 */, bn254_mgpu **out);
void bn254_mgpu_destroy(bn254_mgpu *mg);
int bn254_mgpu_device_count(const bn254_mgpu *mg);
/* the context of entry g (options, bn254_ctx_reserve, bn254_ctx_register_keys ... per device); owned by the handle */
bn254_ctx *bn254_mgpu_ctx(bn254_mgpu *mg, int g);
/* S = ceil(n / G); [lo, hi) of shard g; G * S */
size_t bn254_mgpu_shard_len(const bn254_mgpu *mg, size_t n);
int bn254_mgpu_shard_range(const bn254_mgpu *mg, size_t n, int g, size_t *lo, size_t *hi);
size_t bn254_mgpu_gathered_len(const bn254_mgpu *mg, size_t n);
/* presize every context for batches of n_total items over all devices (bn254_ctx_reserve(ceil(n_total / G)) each) and, when
 * init_collectives != 0, create the RCCL communicators now instead of inside the first *_device call */
int bn254_mgpu_reserve(bn254_mgpu *mg, size_t n_total, int init_collectives);
int bn254_mgpu_synchronize(bn254_mgpu *mg); /* waits for the handle's own streams */
#define BN254_MGPU_OPT_GATHER 1 /* 0 (default) = RCCL when the handle has two or more DISTINCT devices, else peer copies (a one-device handle has
                                   nothing to gather and never loads librccl); 1 = RCCL (an error for duplicate devices — RCCL refuses two
                                   ranks on one device; with one device: the one-rank rehearsal of the RCCL calls); 2 = peer copies */
#define BN254_MGPU_OPT_TIMING 2 /* 1 = record per device the time of its shard's compute and of the collective (bn254_mgpu_last_timing) */
int bn254_mgpu_set_option(bn254_mgpu *mg, int option, int value);
/* per device g of the last call, in ms: compute_ms[g] = its shard's kernels (device entry points: HIP events on its stream; host
 * entry points: the worker's wall clock around staging + kernels + copy-back), collective_ms[g] = the gather / all-reduce as
 * seen on its stream (0 for host entry points).  Synchronises the streams.  Needs BN254_MGPU_OPT_TIMING. */
int bn254_mgpu_last_timing(bn254_mgpu *mg, float *compute_ms /* G */, float *collective_ms /* G */);
/* text of the last RCCL / loader failure on this handle ("" if none); valid until the next call on the handle */
const char *bn254_mgpu_last_error(const bn254_mgpu *mg);

/* status[i] = ECDSA::verify(msg_i, sig_i, pk_i) (src/ecdsa.rs:49-64) for the whole batch, sharded over the devices */
int bn254_mgpu_batch_verify(bn254_mgpu *mg, const uint8_t *msgs, const uint64_t *msg_off /* n+1 */, const uint8_t *sigs /* n*64 */,
                            const uint8_t *pks /* n*128 */, size_t n, uint32_t flags, uint8_t *status /* n */);
int bn254_mgpu_batch_verify_device(bn254_mgpu *mg, const uint8_t *const *d_msgs, const uint64_t *const *d_msg_off,
                                   const uint8_t *const *d_sigs, const uint8_t *const *d_pks, size_t n /* whole batch */, uint32_t flags,
                                   uint8_t *const *d_status_all /* G x gathered_len */, void *const *streams /* G or NULL */);
/* the other verify-shaped host entry points, sharded the same way (same arguments and status bytes as their single-GPU namesakes):
 * from the compressed encodings; with REGISTERED keys (bn254_mgpu_register_keys puts the whole key set on every device; key_status as
 * bn254_ctx_register_keys); the aggregate verify of BASELINE configs[2] — the TUPLES are sharded, messages and pools go to every device,
 * which builds its own subset tables. */
int bn254_mgpu_batch_verify_compressed(bn254_mgpu *mg, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs33, const uint8_t *pks65,
                                       size_t n, uint8_t *status);
int bn254_mgpu_register_keys(bn254_mgpu *mg, const uint8_t *pks /* n_keys*128 */, size_t n_keys, uint32_t flags, uint8_t *key_status /* or NULL */);
/* ... and with every key's proof of possession checked: bn254_ctx_register_keys_pop on every device (each checks the whole set, so no
 * device holds an unproven key as registered); device 0 reports key_status */
int bn254_mgpu_register_keys_pop(bn254_mgpu *mg, const uint8_t *pks /* n_keys*128 */, const uint8_t *pops /* n_keys*64 */, size_t n_keys,
                                 uint32_t flags, uint8_t *key_status /* or NULL */);
int bn254_mgpu_batch_verify_keyed(bn254_mgpu *mg, const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *sigs, const uint32_t *key_idx, size_t n,
                                  uint32_t flags, uint8_t *status);
int bn254_mgpu_batch_aggregate_verify(bn254_mgpu *mg, const uint8_t *msgs, const uint64_t *msg_off, size_t n_msgs, const uint8_t *pk_pool,
                                      size_t n_signers, const uint8_t *sig_pool, const uint32_t *tuple_msg, const uint64_t *tuple_off,
                                      const uint32_t *signer_idx, size_t n, uint32_t flags, uint8_t *status);
/* gt[i], status[i] as bn254_batch_pairing (bn::pairing_batch, src/ecdsa.rs:57); *checksum (optional) = the sum mod 2^64 of all
 * little-endian 64-bit words of the n*384 Gt bytes — BASELINE configs[3]'s cross-shard check.  Device form: d_gt[g] = shard g's
 * n_g*384 bytes; d_checksum[g] (the array or NULL) = 8 bytes on every device receiving the all-reduced (ncclAllReduce, sum,
 * uint64) checksum. */
int bn254_mgpu_batch_pairing(bn254_mgpu *mg, const uint8_t *g1 /* n*k*64 */, const uint8_t *g2 /* n*k*128 */, size_t n, size_t k,
                             uint32_t flags, uint8_t *gt /* n*384 */, uint8_t *status /* n or NULL */, uint64_t *checksum /* or NULL */);
int bn254_mgpu_batch_pairing_device(bn254_mgpu *mg, const uint8_t *const *d_g1, const uint8_t *const *d_g2, size_t n, size_t k,
                                    uint32_t flags, uint8_t *const *d_gt, uint8_t *const *d_status_all, uint64_t *const *d_checksum,
                                    void *const *streams);
/* points[i] = hash_to_try_and_increment(msg_i) (src/hash.rs:29-63) for the whole batch, sharded over the devices */
int bn254_mgpu_batch_hash_to_g1(bn254_mgpu *mg, const uint8_t *msgs, const uint64_t *msg_off, size_t n, uint8_t *points /* n*64 */,
                                uint8_t *status /* n */, uint8_t *tries /* n or NULL */);

/* =====================================================================================================================
 * BN254_DEV_HOOKS — developer hooks, NOT part of the drop-in ABI (bn254_devhooks.hip).  No reference function corresponds to any of
 * them; a binding of the reference's API never needs them.  bn254_debug_* let the parity tests compare every layer of
 * the HIP arithmetic with the oracle; bn254_probe_* are the measurement kernels behind bench.py's roofline figures.  Define
 * BN254_NO_DEV_HOOKS before including this header to hide the declarations.
 * ===================================================================================================================== */
#ifndef BN254_NO_DEV_HOOKS
/* developer options of bn254_ctx_set_option: A/B layouts kept for measurements and for the randomised path's re-check queue, test and
 * measurement knobs.  Same status bytes with every setting; none of them is something a caller of the drop-in ABI should set. */
#define BN254_OPT_SPLIT_MILLER 1 /* 1 = the two Miller loops of a verify in two lanes of different waves (one pairing per lane, one-lane layout only;
                                 default 0) */
#define BN254_OPT_PAIR_LANES 4 /* verify: Miller loop + final exponentiation on lane pairs, two waves per SIMD (default 1); 0 = one lane per verify */
#define BN254_OPT_RAND_ITEMS_PER_LANE 3 /* randomised verify: items per lane in the Miller kernel; 0 = by batch size (default), 1, 2 */
#define BN254_OPT_TRIO_WAVE_ROLES 8 /* octet path, Miller loop: the lane pairs of a verify as WAVES of a workgroup, each with its own instruction
                                     stream (twist point / line product / the halves of f), values exchanged through LDS between barriers:
                                     2 (default) = eight waves per 32 verifies (every Fq6 product split over two waves), 1 = four waves,
                                     0 = four lane pairs of one wave (every pair runs all the linear work).  Same status bytes. */
#define BN254_OPT_HASH_DIRECT_WIDTH 7 /* hash-to-G1 of batches of up to 4096 messages: this many counters of every message are tried at once, in
                                       lanes of one wave, with the square root itself (latency 0.17 ms instead of 0.25); a power of two <= 32,
                                       default 32; 0 = always the filter rounds.  Same points and try counts either way. */
#define BN254_OPT_HASH_SCHEDULE 30 /* hash-to-G1 of batches above 4096 messages: 0 (default) = by size, 1 = always the multi-round filter schedule,
                                    2 = always one wide filter round, then the square roots and the round's few survivors (all their remaining
                                    counters, in lane groups) in one launch.  Same points, statuses and try counts either way. */
#define BN254_OPT_HASH_WIDE_WIDTH 31 /* measurement knob of that schedule (tools/hash_schedule_sweep.py): counters per message in the wide round,
                                      1 .. 64; 0 (default) = chosen by size, 4 .. 8 */
#define BN254_OPT_HASH_TAIL_CHUNK 32 /* test seam: counters a survivor's lane group tries at once in that launch; a power of two, 2 .. 32 (default
                                      32: a second pass of a group has p = 1.3e-9).  Small values let real messages reach the group's loop. */
#define BN254_OPT_NONET_WIDE 16 /* ... and, while the batch is at most one item per SIMD (1 024), on EIGHTEEN lane pairs, one item per wave: the 18
                                 products of a multiplication in one round (default 1; 0 = nine lane pairs at every size) */
#define BN254_OPT_AGG_SORT_BY_MSG 11 /* aggregate verify, batches that use the per-message signature tables: bucket the tuples by message on the
                                      device (counting sort into an index map) so that a workgroup of the aggregation kernel gathers from ONE
                                      message's table; statuses land at the tuples' own indices either way.  Default 1; 0 = the caller's order */
#define BN254_OPT_CLOCK_PROBE 10 /* measurement: 1 = the lane-pair Miller / final-exponentiation kernels and the issue probe record, per workgroup,
                                  shader-clock cycles (s_memtime) and constant-rate ticks (s_memrealtime) between entry and exit, read back by
                                  bn254_ctx_last_clocks: the clock the chip actually sustains under this load (power-limited parts run below
                                  their nominal 2.4 GHz).  Costs two scalar clock reads per workgroup; default 0 */
#define BN254_OPT_HASH_MAX_TRIES 2 /* test knob: counters tried before HashToPointError; 0 = 255 as in src/hash.rs:40 */
#define BN254_OPT_G2_FIXED_BASE 19 /* key derivation (bn254_batch_g2_mul with points = NULL: sk * G2::one()): 1 (default) = 65 additions from a table of the
                                   generator's multiples, built once per context, on a lane pair; 0 = the general 256-step ladder on one lane.  Same bytes. */
#define BN254_OPT_KEY_DEDUP_FORCE_GENERIC 23 /* test hook: the key-dedup route is prepared as usual but the device-side decision always takes the generic
                                             Miller loop (the fallback path of an overflowing or degenerate batch); 2 = the table builder reports a
                                             degenerate line (flags bit 1) for every key it builds — no key bytes that reach one are known —, so the
                                             device takes the decision it takes for such a key: generic loop, nothing cached; default 0 */
#define BN254_OPT_KEY_DEDUP_FOLD 44 /* key dedup: 2 (default) = the keyed Miller loop of the dedup reads each key's plain rows and multiplies the two
                                    table lines of a step into f one at a time, as unit lines (their coefficient at w^3 is one: nine Fq2 products
                                    each), the first step assigned instead of multiplied (k_miller_verify_keyed_unit_pair); 1 = it reads each
                                    key's 22 FOLDED rows — the product of the two
                                    lines of a key that meet with no squaring between them (a nonzero digit's doubling and addition line, the two
                                    closing lines), five Fq2 coefficients per row, built with the key's plain rows and cached with them — and
                                    multiplies one folded element per pair there (k_miller_verify_keyed_fold_pair); 0 = line pair by line pair
                                    (k_miller_verify_keyed_pair).  The rows are built either way.  Same status bytes. */
#define BN254_OPT_KEY_DEDUP_HASH_BITS 24 /* test seam: keep only this many low bits of the key hash of the dedup table (0 = all, default), so that
                                         distinct keys collide: the full 128-byte compare and the probe bound (overflow -> generic loop) */
#define BN254_OPT_AGGD_KEYED_ROUTE 25 /* bn254_batch_aggregate_verify_distinct_keyed: 0 (default) = by size; 1 / 2 = the table-driven slot kernel with
                                    one / two table pairs per lane pair; 3 = the keys expanded into the unkeyed route.  1 and 2 apply on lane pairs
                                    with keys registered.  Same status bytes. */
#define BN254_OPT_AGG_RAND_GROUP_PAIRS 27 /* bn254_batch_aggregate_verify_distinct_keyed_randomized: messages per group of the combined checks (default
                                           1024, at least 1; the number of keys when that is larger).  Same status bytes */
#define BN254_OPT_BITMAP_RAND_GROUP_TUPLES 34 /* bn254_batch_verify_keyed_bitmap_randomized: tuples per group of the combined checks (default 4096, from
                                               the sweeps at 65 536 and 2^20 x 256; at least 1).  Same status bytes */
#define BN254_OPT_BITMAP_ROUTE 29 /* bn254_batch_verify_keyed_bitmap, test hook: 0 (default) = by BN254_OPT_BITMAP_TABLE_MAX_KEYS, 1 = always the subset
                                    tables, 2 = always key by key.  Same status bytes */
#define BN254_OPT_AGG_T4_ROUTE 42 /* aggregate verify, test hook: how the per-message 4-signer signature tables are built: 0 (default) = pair tables, then
                                     quads by batched affine additions (k_pool_pairs_g1 + k_pool_quads_g1); 1 = every entry from the pool
                                     (k_pool_subsets_g1, otherwise only the fallback when the pair table cannot be allocated).  Same tables as
                                     points, same status bytes */
#define BN254_OPT_ASSUME_FREE_MB 18 /* test knob for the automatic slicing rule (BN254_OPT_MAX_CHUNK = 0): price the workspace of a batch against this many MB
                                    of free device memory instead of what hipMemGetInfo reports; 0 = ask the runtime */
/* the routing table of this context as it stands (defaults + options): rows (max_n[i], miller[i], fe[i]) in ascending order of max_n, the last
 * row max_n = UINT64_MAX; miller: 0 lane machine, 1 wave roles, 2 lane pairs; fe: 0 eighteen lane pairs, 1 nine lane pairs, 2 octets, 3 lane
 * pairs.  Returns the number of rows (<= cap) or a negative error.  The parity tests generate every boundary +-1 from it. */
int bn254_debug_route_table(bn254_ctx *ctx, uint64_t *max_n, int *miller, int *fe, int cap);
/* the device-side decision of the key deduplication of the last bn254_batch_verify_device (BN254_OPT_KEY_DEDUP): out = {ran, distinct keys,
 * flags (1 probe overflow, 2 degenerate line), items of the keyed Miller kernel, items of the generic one}; all 0 when the call did not run
 * the dedup.  Synchronises the device. */
int bn254_debug_key_dedup_last(bn254_ctx *ctx, uint32_t out[5]);
/* ... and what that call did with the key cache (BN254_OPT_KEY_CACHE): out = {ran, distinct keys, keys found in the cache, keys built, dropped
 * (bit 0: the new keys did not fit the free rows; bit 1: the cache was emptied before the call — other flags or options, moved buffers, the
 * option at 0)}; a call whose batch the thresholds refuse looks nothing up (hits = built = 0).  Synchronises the device. */
int bn254_debug_key_cache_last(bn254_ctx *ctx, uint32_t out[5]);
/* the Miller-loop line tables as they stand on the device, keys first .. first + count - 1: which = 0 the per-call tables of the key
 * deduplication of the last bn254_batch_verify_device (key ids in the order the device handed them out; rep[k] = the item that represents key
 * k; a key's table is read from the cache row that holds it, so a key that call found cached reads the same as one it built), which = 1 the tables of bn254_ctx_register_keys (rep is not written).  lines: count x 87 x 36 words ([line][c0, c1][re, im][9 limbs],
 * canonical); st / inf (optional): decode status and identity flag per key.  which = 0 after a call whose batch the thresholds refused
 * (more keys than BN254_OPT_KEY_DEDUP_MAX_KEYS, too few items per key, a probe overflow) returns BN254_E_BAD_ARGUMENT and writes nothing: such
 * a call looks no key up and builds no table.  Synchronises the device. */
int bn254_debug_key_tables(bn254_ctx *ctx, int which, size_t first, size_t count, int32_t *lines, uint32_t *rep, uint8_t *st, uint8_t *inf);
/* ... and the FOLDED rows of the keys of the last key deduplication (BN254_OPT_KEY_DEDUP_FOLD), keys first .. first + count - 1 in the order of
 * bn254_debug_key_tables(which = 0), each read from the cache row that holds it: rows = count x 22 x 90 words ([row][K0 .. K4][re, im][9
 * limbs], canonical).  BN254_E_BAD_ARGUMENT, nothing written, where bn254_debug_key_tables(0, ..) returns it.  Synchronises the device. */
int bn254_debug_key_fold_tables(bn254_ctx *ctx, size_t first, size_t count, int32_t *rows);
/* the tables of the registered pools (bn254_ctx_register_pools) as they stand on the device: which = the context's pool index — 0 the decoded
 * key pool (n_signers entries), 1 the decoded signature pool (n_msgs * n_signers), 2 H(m) (n_msgs), 3 T8 keys (entry g * 256 + mask), 4 T4
 * signatures ((m * groups4 + g) * 16 + mask), 5 T16 keys (k * 65536 + mask), 6 T8 signatures ((m * n_groups + g) * 256 + mask), 7 T2 signatures
 * ((m * 2 * groups4 + pair) * 4 + mask).  points: entries first .. first + count - 1 as canonical big-endian bytes, 64 per G1 entry, 128 per G2
 * entry (which = 0, 3, 5), all-zero for an entry flagged as the identity (the tables store non-canonical words: the hook canonicalises);
 * flags: the raw status bytes (0x80 = identity; in the decoded pools the low bits are the decode status, under which the coordinates are
 * the generator's).  QUERY FORM, which = -1: points receives five uint64_t (40 bytes, 8-byte aligned) {n_groups, groups4, wide2, wide1, the
 * builder of the T4 signatures: 0 none, 1 pairs + quads, 2 k_pool_subsets_g1}; first, count and flags are not used.
 * BN254_E_BAD_ARGUMENT when no registration is valid (none yet, or a call with raw pools since), when the table was not built, and when
 * first + count runs past the table.  Synchronises the context. */
int bn254_debug_agg_tables(bn254_ctx *ctx, int which, size_t first, size_t count, uint8_t *points, uint8_t *flags);
/* what the last bn254_batch_aggregate_verify_distinct_keyed_randomized[_device] did: out = {1 if it took the randomised route, groups that
 * reached the check, table pairs of all group checks, failed groups, aggregates re-checked, groups of one aggregate (r = 1)}; all 0 when it
 * took the exact route.  Synchronises the device. */
int bn254_debug_agg_rand_last(bn254_ctx *ctx, uint64_t out[6]);
/* the G1 side of the group checks of that call, read from where it left them (valid until the next call on the context; the call itself
 * does nothing extra for this).  dims = {groups = m / G + 1 (those with no aggregate included), table pairs of all groups}; dims = {0, 0}
 * when the call took the exact route.  With group_cap >= groups and pair_cap >= table pairs also, per group g: nagg[g] = its aggregates
 * at the check, verdict[g] = the status byte of its check (0 / 9; meaningful where nagg[g] != 0), s_g = S_g = sum r_i sigma_i (64 bytes
 * affine, zeros = the identity), first_pair[g] .. first_pair[g + 1] = its table pairs (groups + 1 entries), and per table pair its key index
 * and its point sum r_i H(m_j) over the group's entries of that key (64 bytes).  Otherwise only dims is written.  Synchronises the device. */
int bn254_debug_agg_rand_sums(bn254_ctx *ctx, uint64_t dims[2], size_t group_cap, size_t pair_cap, uint32_t *nagg, uint8_t *verdict,
                              uint8_t *s_g /* groups*64 */, uint64_t *first_pair /* groups+1 */, uint32_t *pair_key, uint8_t *pair_point /* pairs*64 */);
/* what the last bn254_batch_collect_keyed_bitmap_randomized[_device] did, summed over its slices (the kernels count): out = {slices that took
 * the randomised route, groups checked, groups that failed, shares re-checked exactly}; all 0 when the call took the exact route.
 * Synchronises the device. */
int bn254_debug_collect_rand_last(bn254_ctx *ctx, uint64_t out[4]);
/* what the last bn254_batch_collect_keyed_bitmap_optimistic[_device] did, counted by the call's own kernels and summed over its slices: out =
 * {tuples checked optimistically, tuples that passed, tuples sent to the exact route (failed, a duplicate, or below the per-tuple minimum),
 * shares verified exactly}; all 0 when the call as a whole took the exact route.  Synchronises the device. */
int bn254_debug_collect_opt_last(bn254_ctx *ctx, uint64_t out[4]);
/* what the last bn254_batch_threshold_combine_keyed_optimistic[_device] did, counted by the call's own kernels: out = {tuples checked under the
 * group key, tuples that passed, tuples sent the exact way (failed, a duplicate, or fewer candidates than the threshold), shares verified
 * exactly}; all 0 ("did not run") after any call that did not take the optimistic route.  Synchronises the device. */
int bn254_debug_threshold_opt_last(bn254_ctx *ctx, uint64_t out[4]);
/* what the last bn254_batch_merge_keyed_bitmap_optimistic[_device] did, counted by the call's own kernels and summed over its slices: out =
 * {tuples checked optimistically, tuples that passed, tuples sent the exact way (failed, or an overlap), partials verified exactly}; all 0
 * ("did not run") after any call that did not take the route — the exact merge and the collect calls included.  Synchronises the device. */
int bn254_debug_merge_opt_last(bn254_ctx *ctx, uint64_t out[4]);
/* what the last bn254_batch_verify_keyed_bitmap_randomized[_device] did (its last slice): out = {1 if it took the randomised route, groups that
 * reached the check, table pairs of all group checks (S_g's included), failed groups, tuples re-checked, groups of one tuple (r = 1)}; all 0
 * when it took the exact route.  Synchronises the device. */
int bn254_debug_bitmap_rand_last(bn254_ctx *ctx, uint64_t out[6]);
/* the G1 side of the group checks of that call, read from where it left them, in the format of bn254_debug_agg_rand_sums: dims = {groups =
 * ceil(n / G), table pairs of all groups}; per group its tuples at the check, the status byte of its check, S_g, and its (key index, T_{g,j})
 * pairs in key order — one per key with a contributor, zeros = a sum that came out as the identity.  The call itself launches nothing for
 * this.  Synchronises the device. */
int bn254_debug_bitmap_rand_sums(bn254_ctx *ctx, uint64_t dims[2], size_t group_cap, size_t pair_cap, uint32_t *nagg, uint8_t *verdict,
                                 uint8_t *s_g /* groups*64 */, uint64_t *first_pair /* groups+1 */, uint32_t *pair_key, uint8_t *pair_point /* pairs*64 */);
/* test hooks: element-wise field/tower operations on byte-encoded operands, used by the parity
 * tests to compare each layer of the HIP arithmetic with the oracle.
 *   op: 0 mul, 1 add, 2 sub, 3 inverse(a), 4 square(a), 5 sqrt(a) (status 6 if none)   [Fq, 32 B]
 *   fp12 op: 0 mul, 1 square, 2 inverse, 3 conj, 4 frobenius^1, 5 ^2, 6 ^3, 7 cyclotomic square,
 *            8 final exponentiation                                                    [384 B] */
int bn254_debug_fp_op(bn254_ctx *ctx, int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out, uint8_t *status);
int bn254_debug_fp12_op(bn254_ctx *ctx, int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out);
/* ... and in Fr, arithmetic mod the group order (bn254_fr.h), on 32-byte big-endian operands, reduced mod r on load as
 * bn254_batch_g1_mul(reduce_scalar = 1) reduces a scalar; out = 32 B big-endian, in [0, r).
 *   op: 0 mul, 1 add, 2 sub (b required), 3 neg(a), 4 inverse(a) (0 gives 0), 5 a itself through Montgomery form and back,
 *       6 the low 32 bits of a (its last four bytes) through the uint32_t load */
int bn254_debug_fr_op(bn254_ctx *ctx, int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out /* n*32 */);
/* the Lagrange coefficients at zero of bn254_batch_threshold_combine_keyed, the evaluation points given directly (so a test can use points up
 * to 2^32 - 1 without registering that many keys): segment i holds the points x[seg_off[i] .. seg_off[i+1]), and out[32 j] is the
 * coefficient of point j within its segment, prod x_k / prod (x_k - x_j) mod r over the segment's other points.  The points of a segment
 * must be distinct and non-zero (a repeated point gives 0).  seg_off[0] == 0, non-decreasing. */
int bn254_debug_lagrange_at_zero(bn254_ctx *ctx, const uint32_t *x /* m */, const uint64_t *seg_off /* n+1 */, size_t n, uint8_t *out /* m*32 */);
/* the coefficients c_0 .. c_n_keys-1 of bn254_ctx_check_dealing's degree check for n_keys keys, 1 <= threshold <= n_keys and the seed, by
 * the call's own kernels; independent of any registration */
int bn254_debug_dealing_coefficients(bn254_ctx *ctx, size_t n_keys, uint32_t threshold, const uint8_t *seed32,
                                     uint8_t *out /* n_keys*32, big-endian, reduced */);
/* the final exponentiation of ECDSA::verify / bn::pairing_batch (src/ecdsa.rs:57-59) on caller-supplied LIMB vectors — n x 12 coefficients
 * (Gt order) x 9 int32 limbs, value = sum limb_k 2^(29 k) in Montgomery form (R = 2^261) — in the layout named: 0 one lane per item, exact
 * exponent, gt = canonical Gt bytes | 1 lane pairs, exact, gt | 2 lane pairs, the == one chain | 3 lane octets (straight-line chains below
 * 128 items, accumulator machine from 128 on) | 4 nine lane pairs per item | 5 one lane, the == one chain | 6 eighteen lane pairs per item (one per wave).  status[i] = 0 (the value is one) or 9.
 * Exists so that the parity tests can hand every layout NON-CANONICAL representatives with extreme balanced digits — what the interval
 * tracker's contract for a Miller value allows (limbs 0..7 in [-2^28, 2^28], |value| <= 0.5215 q) but no byte decoder produces. */
int bn254_debug_final_exp_limbs(bn254_ctx *ctx, int layout, const int32_t *limbs /* n*108 */, size_t n, uint8_t *gt /* n*384, layouts 0 / 1, or NULL */,
                                uint8_t *status /* n */);
/* what ONE pass of the try loop of hash_to_try_and_increment does with a chosen 256-bit digest value h (32 B
 * big-endian each) instead of SHA-256(msg || ctr): the h >= 5q rule (src/hash.rs:49-51), mod_u256's strict '>'
 * (src/utils.rs:27-37) and G1::from_compressed(0x02 || x) (src/utils.rs:56-63).  status 0: out = the point; 1: the
 * loop would move to the next counter (out = zeros).  Exists because h = k*q has no known preimage. */
int bn254_debug_hash_candidate(bn254_ctx *ctx, const uint8_t *h /* n*32 */, size_t n, uint8_t *out /* n*64 */, uint8_t *status);
/* the Jacobi symbol of the hash filter (bn254_hash.h: u256_is_square_mod_q, the test every counter of hash-to-G1 meets before its square
 * root), element-wise, one lane per item, on 32-byte big-endian integers.  A whole hash only ever hands the filter x^3 + 3 of a digest — a
 * uniformly random value; this hook hands it chosen ones.
 *   mode 0: a (an integer below q) goes straight into the filter.  out_flags[i] bit 0 = its answer (1: a square mod q, zero included).
 *           a >= q: bit 7 and nothing else.
 *   mode 1: a = a candidate x below q, through x^3 + 3 and the conversion to a plain integer exactly as the filter round does.  out_value =
 *           the integer the filter is handed; bit 0 = the filter's answer; bit 1 = whether the square root behind the filter yields a
 *           point (the two bits agree, or a message would get the wrong counter).  a >= q: bit 7 and nothing else.
 *   mode 2: the symbol (a / b) of the caller's odd b >= 3 and a < b, through the same passes in the same phases under the same budget
 *           (a modulus of 64, 128 or 192 bits enters the narrower phases directly, which no value mod q does).  out_flags[i] = 0: symbol
 *           +1, 1: symbol -1, 2: symbol 0 (a and b share a factor).  An even b, b < 3 or a >= b: bit 7 and nothing else.
 * out_value in modes 0 and 2 = a as the passes received it; zeros where bit 7 is set.  b is read in mode 2 only (may be NULL otherwise).
 * BN254_E_BAD_ARGUMENT for another mode or a missing buffer; n == 0 returns 0. */
int bn254_debug_jacobi(bn254_ctx *ctx, int mode, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out_value /* n*32 */, uint8_t *out_flags /* n */);
/* ONE Fq / Fq2 primitive of the field layer (bn254_field.h, bn254_fp2_pair.h) per item on RAW limb vectors: an operand is 18 int32 — the 9
 * limbs of the real coefficient, then of the imaginary one, value = sum limb_k 2^(29 k), Montgomery form (R = 2^261) — handed to the
 * primitive as it stands: no decoding, no carry, no range check.  The result is 18 int32 as the primitive left them (not canonicalised)
 * and one flag byte for the predicates.  Exists because the field layer is lazy: the interval tracker of the host builds proves the
 * formulas under a postcondition it ASSUMES for every primitive, and the device runs other source than the host in the pair layout (DPP
 * exchanges, the asm prologue of the squaring, the folded negation of the multiplication by xi) — this hook hands the device primitives
 * chosen in-contract limb vectors at the contract's edge, which no byte decoder produces (tests/fq_limb_cases.py).  The caller keeps every
 * operand inside the primitive's contract; outside it the limbs returned mean nothing (nothing else can happen: the kernels touch no
 * memory but these buffers).
 *   layout 0: one lane per item, the classic fp2_* / fp_* (bn254_devhooks.hip) | 1: one lane PAIR per item, even lane the real and odd lane the
 *             imaginary coefficient, in the translation unit and workgroup shape of the lane-pair kernels (bn254_pair.hip).  The octet,
 *             quad, nonet and lane-machine layouts have no entry here: they run these same per-lane primitives, and their exchanges are
 *             entered by bn254_debug_final_exp_limbs with adversarial limb vectors.
 *   operands: n x 4 x 18 (a, b, c, d of item i at 72 i); coef: n x 4 int32 (k0 .. k3).  Operands and factors an op does not name are ignored.
 *   op:  0 a + b | 1 a - b | 2 -a | 3 2 a | 4 conj a | 5 i a | 6 k0 != 0 ? a : b                                (lazy: limb-wise)
 *        7 norm a | 8 reduce_weak a | 9 lin2_reduce: k0 a + k1 b | 10 lin4_reduce: k0 a + k1 b + k2 c + k3 d (layout 0: coefficient-wise) |
 *        11 8 a (mul8_spread) | 12 xi a | 13 xi norm(a)     (xi = 9 + i)
 *        14 a b | 15 a^2 | 16 a times the real coefficient of b (mul_fp) | 17 1 / a (0 gives 0)
 *        18 canon, coefficient-wise | 19 to_u256, coefficient-wise: the 8 words of the plain integer in limbs 0..7, limb 8 = 0 |
 *        20 flag = a is zero | 21 flag = a equals b | 22 flag = u512_greater: a above b in the order (im, re) of the canonical integers |
 *        23 norm_floor, coefficient-wise.       Ops 20 .. 22 return zero limbs.
 *   (fp2_mul_sum, the sum of N products under one reduction, is instantiated only by the BN_PAIR_FP6_LAZY measurement build, not by this
 *   library: it has no op.)
 * flags[i] = 0 / 1; in layout 1 both lanes of the pair form the answer, and bit 7 is set if they ever disagree.
 * BN254_E_BAD_ARGUMENT for another layout or op, for a missing buffer with n > 0, and for n above 14 913 080 (the operands of a call stay below
 * 4 GiB); n == 0 returns 0. */
int bn254_debug_fq2_limbs(bn254_ctx *ctx, int layout, int op, const int32_t *operands /* n*72 */, const int32_t *coef /* n*4 */, size_t n,
                          int32_t *out /* n*18 */, uint8_t *flags /* n */);
/* un-exponentiated Miller-loop value of each single pair (debugging aid) */
int bn254_debug_miller_loop(bn254_ctx *ctx, const uint8_t *g1, const uint8_t *g2, size_t n, uint8_t *f /* n*384 */);

/* calibration probe for the roofline figures of bench.py: sustained wave-instructions per second of one VALU
 * instruction (op 0 v_mad_u64_u32, 1 v_add_u32, 2 v_mul_lo_u32; 16 independent chains) with waves_per_simd (1..8)
 * waves on every SIMD of the device; n_simd (optional) = SIMD count.  Synchronises the context's stream. */
int bn254_probe_issue_rate(bn254_ctx *ctx, int op, int waves_per_simd, double *wave_inst_per_s, int *n_simd);
/* measurement: duration in ms of a kernel that runs ONLY the field-product calls of one verify's Miller loop (mode 0: 3 219 dual
 * products, 435 squarings, 348 scalings per lane) or final exponentiation (mode 1: 945 dual products, 1 701 squarings) for n lane pairs —
 * no tower additions, carries, twist point or LDS traffic — on the launch shape of those kernels: a floor for any arrangement of the
 * code around the product leaves.  n <= the size of the workspace.  With BN254_OPT_CLOCK_PROBE its clock lands in slot [2].
 * Modes 2 / 3: 3 219 dual products with the leaf inlined into the loop / called — what the calling convention costs per product.
 * Modes 4 / 5: the product counts of modes 0 / 1 as FOUR independent chains per lane (in modes 0 / 1 every product waits for its
 * predecessor, which a lone wave per SIMD cannot hide): the floor to quote is the smaller of the two.  Modes 6 / 7: controls for mode 4 —
 * the same loop with one chain / two chains. */
int bn254_probe_leaf_floor(bn254_ctx *ctx, size_t n, int mode, float *ms);
/* measurement: duration in ms of the final exponentiation's accumulator machine (the interpreter of the lane-pair kernel) running a
 * caller-supplied program of n_steps (opcode, argument) byte pairs — 1 LOAD slot, 2 STORE slot, 3 CSQR, 4 MUL slot, 5 CONJ, 6 FROB 1..3,
 * 7 INV; slots 0..9 — for n lane pairs on the values the last verify left in the workspace.  Programs of one operation kind give the cost
 * of that operation in place (bench.py: roofline.final_exp_split); results are not meaningful values. */
int bn254_probe_fe_program(bn254_ctx *ctx, size_t n, const uint8_t *prog, size_t n_steps, float *ms);
#endif /* BN254_NO_DEV_HOOKS */

#ifdef __cplusplus
}
#endif
#endif /* BN254_HIP_H */
