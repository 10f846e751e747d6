// bn254.hpp — C++ host-side mirror of the reference's public API (/root/reference/src/lib.rs:60-63)
// over the C ABI of libbn254hip.so (include/bn254_hip.h).  Header-only; link with -lbn254hip.
//
//   bn254::ECDSA::sign / verify / batch_verify      /root/reference/src/ecdsa.rs:26-35, :49-64 (+ new batch entry)
//   bn254::ECDSA::aggregate_verify / batch_aggregate_verify_distinct   (new: aggregates over distinct messages)
//   bn254::ECDSA::aggregate_verify_keyed / batch_aggregate_verify_distinct_keyed   (... against registered keys)
//   bn254::ECDSA::verify_keyed_signers / batch_verify_keyed_signers                 (one message, an aggregated signature, the signers' indices)
//   bn254::ECDSA::batch_aggregate_verify_distinct_keyed_randomized                  (... with the group checks combined)
//   bn254::ECDSA::aggregate_public_key_signers / verify_keyed_signers_export / register_key_weights / signers_weight   (what a bitmap call returns)
//   bn254::format_pairing_check_values / _uncompressed_values / _keyed_signers        src/utils.rs:197-239
//   bn254::check_public_keys                        /root/reference/src/ecdsa.rs:78-93
//   bn254::PrivateKey / PublicKey / PublicKeyG1 / Signature   /root/reference/src/types.rs:13,81,151,222
//   bn254::Error                                    /root/reference/src/error.rs:6-29
//
// Points are held as the reference's uncompressed encodings (identity = all-zero bytes); every
// group operation runs on the GPU.  A failed verification throws Error{VerificationFailed}, like
// the reference returns Err(Error::VerificationFailed) (not Ok(false)).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bn254_hip.h"

namespace bn254 {

enum class ErrorKind : uint8_t {   // the status codes of include/bn254_hip.h = 1 + the variant's index in /root/reference/src/error.rs:6-29
  HashToPointError = BN254_ERR_HASH_TO_POINT, IndexOutOfBounds = BN254_ERR_INDEX_OUT_OF_BOUNDS, InvalidEncoding = BN254_ERR_INVALID_ENCODING,
  InvalidGroupPoint = BN254_ERR_INVALID_GROUP_POINT, InvalidLength = BN254_ERR_INVALID_LENGTH, NotMemberError = BN254_ERR_NOT_MEMBER,
  ToAffineConversion = BN254_ERR_TO_AFFINE_CONVERSION, PointInJacobian = BN254_ERR_POINT_IN_JACOBIAN,
  VerificationFailed = BN254_ERR_VERIFICATION_FAILED, SerializationError = BN254_ERR_SERIALIZATION, HexDecodeFailed = BN254_ERR_HEX_DECODE_FAILED
};
struct Error : std::runtime_error {
  ErrorKind kind;
  explicit Error(ErrorKind k) : std::runtime_error("bn254 error " + std::to_string((int)k)), kind(k) {}
};
struct NativeError : std::runtime_error {
  int rc;
  NativeError(const char* fn, int r) : std::runtime_error(std::string(fn) + " failed, rc=" + std::to_string(r)), rc(r) {}
};
inline void check_rc(const char* fn, int rc) { if (rc != 0) throw NativeError(fn, rc); }
inline void check_status(uint8_t s) { if (s != 0) throw Error((ErrorKind)s); }
// what ECDSA::reshare_commitments returns, and what it throws when too few dealers qualify (Error(VerificationFailed) with the details)
struct ReshareFailed : Error {
  std::vector<uint8_t> statuses;       // per dealer in index order: 0 or its ErrorKind
  std::vector<uint32_t> qualified;     // the key indices of the dealers that did qualify
  ReshareFailed(std::vector<uint8_t> st, std::vector<uint32_t> q) : Error(ErrorKind::VerificationFailed), statuses(std::move(st)), qualified(std::move(q)) {}
};

class Engine {   // one per GPU; not thread-safe (one thread at a time per context)
 public:
  explicit Engine(int device = 0) { check_rc("bn254_ctx_create", bn254_ctx_create(device, &ctx_)); }
  ~Engine() { bn254_ctx_destroy(ctx_); }
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  bn254_ctx* raw() const { return ctx_; }
  // a BN254_OPT_* of include/bn254_hip.h, e.g. OPT_MERGE_OPT_MIN_PARTS below
  void set_option(int option, int value) { check_rc("bn254_ctx_set_option", bn254_ctx_set_option(ctx_, option, value)); }
  // merge_keyed_signers_optimistic: calls with fewer partials take the exact merge, same bytes; 0 = no lower bound
  static constexpr int OPT_MERGE_OPT_MIN_PARTS = BN254_OPT_MERGE_OPT_MIN_PARTS;
  static Engine& default_engine() { static Engine e(0); return e; }
 private:
  bn254_ctx* ctx_ = nullptr;
};

// All the GPUs of a node behind one handle (include/bn254_hip.h, section "Multi-GPU"): the batch is cut into contiguous shards, one per
// device entry, each verified by that device's own context from its own parked worker thread; ECDSA::batch_verify(gpus, ...) below.
class Gpus {
 public:
  explicit Gpus(const std::vector<int>& devices) { check_rc("bn254_mgpu_create", bn254_mgpu_create(devices.data(), (int)devices.size(), &mg_)); }
  ~Gpus() { bn254_mgpu_destroy(mg_); }
  Gpus(const Gpus&) = delete;
  Gpus& operator=(const Gpus&) = delete;
  bn254_mgpu* raw() const { return mg_; }
  int count() const { return bn254_mgpu_device_count(mg_); }
 private:
  bn254_mgpu* mg_ = nullptr;
};

struct PrivateKey {   // PrivateKey(Fr): 32-byte big-endian scalar, reduced mod r on use
  std::array<uint8_t, 32> bytes{};
  static PrivateKey try_from(const uint8_t* data, size_t len) {
    if (len != 32) throw Error(ErrorKind::InvalidLength);          // types_test.rs:29-46
    PrivateKey k; std::memcpy(k.bytes.data(), data, 32); return k;
  }
};

template <size_t N> struct PointBytes {
  std::array<uint8_t, N> raw{};
  bool is_identity() const { for (auto b : raw) if (b) return false; return true; }
  const std::array<uint8_t, N>& to_uncompressed() const {
    if (is_identity()) throw Error(ErrorKind::PointInJacobian);    // utils.rs:163,184
    return raw;
  }
};

struct Signature : PointBytes<64> {
  static Signature from_uncompressed(const uint8_t* data, size_t len, Engine& e = Engine::default_engine()) {
    if (len != 64) throw Error(ErrorKind::InvalidLength);          // utils.rs:120
    Signature s; std::memcpy(s.raw.data(), data, 64);
    if (s.is_identity()) throw Error(ErrorKind::InvalidGroupPoint);
    uint8_t zero[64] = {0}, out[64], st = 0;
    check_rc("bn254_batch_g1_add", bn254_batch_g1_add(e.raw(), s.raw.data(), zero, 1, out, &st));
    check_status(st);
    return s;
  }
  static Signature from_compressed(const uint8_t* data, size_t len, Engine& e = Engine::default_engine()) {   // types.rs:233-237
    if (len != 33) throw Error(ErrorKind::InvalidEncoding);
    Signature s; uint8_t st = 0;
    check_rc("bn254_batch_g1_decompress", bn254_batch_g1_decompress(e.raw(), data, 1, s.raw.data(), &st));
    check_status(st);
    return s;
  }
  std::array<uint8_t, 33> to_compressed() const {                  // utils.rs:84-104
    if (is_identity()) throw Error(ErrorKind::PointInJacobian);
    std::array<uint8_t, 33> o{};
    o[0] = (raw[63] & 1) ? 3 : 2;
    std::memcpy(o.data() + 1, raw.data(), 32);
    return o;
  }
  Signature operator+(const Signature& o) const {                  // types.rs:264-270
    Signature r; uint8_t st = 0;
    check_rc("bn254_batch_g1_add", bn254_batch_g1_add(Engine::default_engine().raw(), raw.data(), o.raw.data(), 1, r.raw.data(), &st));
    check_status(st);
    return r;
  }
};
// A signature as it arrives off the wire — 0x02 / 0x03 || x, 33 bytes — and NOT yet decoded: the registered-key calls of ECDSA take it as it is
// and decompress on the device, inside the call (include/bn254_hip.h: BN254_FLAG_G1_COMPRESSED).  An encoding that does not decompress gets the
// ErrorKind Signature::from_compressed would throw as its status and is never verified, taken or counted.
struct CompressedSignature {
  std::array<uint8_t, 33> raw{};
  static CompressedSignature from_bytes(const uint8_t* data, size_t len) {
    if (len != 33) throw Error(ErrorKind::InvalidEncoding);        // as Signature::from_compressed
    CompressedSignature s; std::memcpy(s.raw.data(), data, 33);
    return s;
  }
};
// the flag a call passes for an input array of such points
template <class Sig> constexpr uint32_t g1_input_flag() { return std::tuple_size<decltype(Sig::raw)>::value == 33 ? BN254_FLAG_G1_COMPRESSED : 0u; }

struct PublicKeyG1 : PointBytes<64> {
  static PublicKeyG1 from_private_key(const PrivateKey& k, Engine& e = Engine::default_engine()) {   // types.rs:155-157
    PublicKeyG1 r; uint8_t st = 0;       // points = nullptr: G1::one(), the fixed-base table of the generator
    check_rc("bn254_batch_g1_mul", bn254_batch_g1_mul(e.raw(), nullptr, k.bytes.data(), 1, 1, r.raw.data(), &st));
    check_status(st);
    return r;
  }
};
struct PublicKey : PointBytes<128> {
  static PublicKey from_private_key(const PrivateKey& k, Engine& e = Engine::default_engine()) {     // types.rs:85-87
    PublicKey r; uint8_t st = 0;
    check_rc("bn254_batch_g2_mul", bn254_batch_g2_mul(e.raw(), nullptr, k.bytes.data(), 1, 1, r.raw.data(), &st));
    check_status(st);
    return r;
  }
  static PublicKey from_compressed(const uint8_t* data, size_t len, Engine& e = Engine::default_engine()) {   // types.rs:91-93
    if (len != 65) throw Error(ErrorKind::InvalidEncoding);
    PublicKey r; uint8_t st = 0;
    check_rc("bn254_batch_g2_decompress", bn254_batch_g2_decompress(e.raw(), data, 1, r.raw.data(), &st));
    check_status(st);
    return r;
  }
  PublicKey operator+(const PublicKey& o) const {                  // types.rs:126-132
    PublicKey r; uint8_t st = 0;
    check_rc("bn254_batch_g2_add", bn254_batch_g2_add(Engine::default_engine().raw(), raw.data(), o.raw.data(), 1, r.raw.data(), &st));
    check_status(st);
    return r;
  }
  bool operator==(const PublicKey& o) const { return raw == o.raw; }
};

struct ECDSA {
  static Signature sign(const std::vector<uint8_t>& message, const PrivateKey& k, Engine& e = Engine::default_engine()) {
    uint64_t off[2] = {0, message.size()};
    Signature s; uint8_t st = 0;
    check_rc("bn254_batch_sign", bn254_batch_sign(e.raw(), message.data(), off, k.bytes.data(), 1, s.raw.data(), &st));
    check_status(st);
    return s;
  }
  static void verify(const std::vector<uint8_t>& message, const Signature& s, const PublicKey& pk, Engine& e = Engine::default_engine()) {
    uint64_t off[2] = {0, message.size()};
    uint8_t st = 0;
    check_rc("bn254_batch_verify", bn254_batch_verify(e.raw(), message.data(), off, s.raw.data(), pk.raw.data(), 1, 0, &st));
    check_status(st);
  }
  // result[i] == 0 iff verify(messages[i], signatures[i], public_keys[i]) succeeds, else the ErrorKind it would throw
  static std::vector<uint8_t> batch_verify(const std::vector<std::vector<uint8_t>>& messages, const std::vector<Signature>& signatures,
                                           const std::vector<PublicKey>& public_keys, Engine& e = Engine::default_engine()) {
    size_t n = messages.size();
    if (signatures.size() != n || public_keys.size() != n) throw Error(ErrorKind::InvalidLength);
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<uint8_t> msgs, sigs(n * 64), pks(n * 128), status(n, 0);
    for (size_t i = 0; i < n; ++i) {
      off[i] = msgs.size();
      msgs.insert(msgs.end(), messages[i].begin(), messages[i].end());
      std::memcpy(&sigs[64 * i], signatures[i].raw.data(), 64);
      std::memcpy(&pks[128 * i], public_keys[i].raw.data(), 128);
    }
    off[n] = msgs.size();
    check_rc("bn254_batch_verify", bn254_batch_verify(e.raw(), msgs.data(), off.data(), sigs.data(), pks.data(), n, 0, status.data()));
    return status;
  }
  // Aggregate signature over DISTINCT messages (the IRTF BLS draft's AggregateVerify): signature = the sum of the signatures of
  // public_keys[j] on messages[j].  Throws the Error of the first failing check (signature, keys, messages, then VerificationFailed);
  // include/bn254_hip.h: bn254_batch_aggregate_verify_distinct.  Assumes a proof of possession of every key (verify_possession,
  // register_keys_proven below); distinct messages are not enforced.
  struct Aggregate { std::vector<std::vector<uint8_t>> messages; Signature signature; std::vector<PublicKey> public_keys; };
  static void aggregate_verify(const std::vector<std::vector<uint8_t>>& messages, const Signature& signature, const std::vector<PublicKey>& public_keys,
                               Engine& e = Engine::default_engine()) {
    check_status(batch_aggregate_verify_distinct({Aggregate{messages, signature, public_keys}}, e)[0]);
  }
  // result[i] == 0 iff aggregate_verify on aggregates[i] succeeds, else the ErrorKind it would throw
  static std::vector<uint8_t> batch_aggregate_verify_distinct(const std::vector<Aggregate>& aggregates, Engine& e = Engine::default_engine()) {
    const size_t n = aggregates.size();
    std::vector<uint64_t> msg_off(1, 0), agg_off(1, 0);
    std::vector<uint8_t> msgs, pks, sigs(n * 64), status(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const Aggregate& a = aggregates[i];
      if (a.messages.size() != a.public_keys.size()) throw Error(ErrorKind::InvalidLength);
      for (size_t j = 0; j < a.messages.size(); ++j) {
        msgs.insert(msgs.end(), a.messages[j].begin(), a.messages[j].end());
        msg_off.push_back(msgs.size());
        pks.insert(pks.end(), a.public_keys[j].raw.begin(), a.public_keys[j].raw.end());
      }
      agg_off.push_back(msg_off.size() - 1);
      std::memcpy(&sigs[64 * i], a.signature.raw.data(), 64);
    }
    const size_t m = msg_off.size() - 1;
    check_rc("bn254_batch_aggregate_verify_distinct", bn254_batch_aggregate_verify_distinct(e.raw(), msgs.data(), msg_off.data(), pks.data(), m, sigs.data(),
                                                                                            agg_off.data(), n, 0, status.data()));
    return status;
  }
  // the same over all the GPUs of a node: shard g of the batch on device entry g, statuses straight into result's slices
  static std::vector<uint8_t> batch_verify(Gpus& gpus, const std::vector<std::vector<uint8_t>>& messages, const std::vector<Signature>& signatures,
                                           const std::vector<PublicKey>& public_keys) {
    size_t n = messages.size();
    if (signatures.size() != n || public_keys.size() != n) throw Error(ErrorKind::InvalidLength);
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<uint8_t> msgs, sigs(n * 64), pks(n * 128), status(n, 0);
    for (size_t i = 0; i < n; ++i) {
      off[i] = msgs.size();
      msgs.insert(msgs.end(), messages[i].begin(), messages[i].end());
      std::memcpy(&sigs[64 * i], signatures[i].raw.data(), 64);
      std::memcpy(&pks[128 * i], public_keys[i].raw.data(), 128);
    }
    off[n] = msgs.size();
    check_rc("bn254_mgpu_batch_verify", bn254_mgpu_batch_verify(gpus.raw(), msgs.data(), off.data(), sigs.data(), pks.data(), n, 0, status.data()));
    return status;
  }
  // Keyed verify: a validator set registered once (PublicKey::from_uncompressed per key, types.rs:96-99, plus the key's Miller-loop
  // lines tabulated in HBM), then tuples name their key by index.  register_keys: result[j] == 0 or the ErrorKind of key j.
  static std::vector<uint8_t> register_keys(const std::vector<PublicKey>& keys, Engine& e = Engine::default_engine()) {
    std::vector<uint8_t> pks(keys.size() * 128), status(keys.size(), 0);
    for (size_t j = 0; j < keys.size(); ++j) std::memcpy(&pks[128 * j], keys[j].raw.data(), 128);
    check_rc("bn254_ctx_register_keys", bn254_ctx_register_keys(e.raw(), pks.data(), keys.size(), 0, status.data()));
    return status;
  }
  // PROOFS OF POSSESSION (include/bn254_hip.h: BN254_POP_TAG, bn254_batch_pop_prove / _verify, bn254_ctx_register_keys_pop) — what the
  // same-message aggregate calls below assume of the registered keys.  The proof of a key is its holder's signature on BN254_POP_TAG || pk,
  // pk the key's 128 uncompressed bytes.  Two caller rules: a signer must refuse application messages that begin with BN254_POP_TAG, and a
  // proof is bound to the key's encoding bytes.  The identity is refused, as a key and as a proof (BN254_FLAG_REJECT_IDENTITY).
  static Signature prove_possession(const PrivateKey& k, Engine& e = Engine::default_engine()) {
    uint8_t pk[128], st = 0;
    Signature pop;
    check_rc("bn254_batch_pop_prove", bn254_batch_pop_prove(e.raw(), k.bytes.data(), 1, pk, pop.raw.data(), &st));
    check_status(st);
    return pop;
  }
  // result[j] == 0 iff proofs[j] is the proof of possession of keys[j], else the ErrorKind verify_possession would throw
  static std::vector<uint8_t> batch_verify_possession(const std::vector<PublicKey>& keys, const std::vector<Signature>& proofs,
                                                      Engine& e = Engine::default_engine()) {
    const size_t n = keys.size();
    if (proofs.size() != n) throw Error(ErrorKind::InvalidLength);
    std::vector<uint8_t> pks(n * 128), pops(n * 64), status(n, 0);
    for (size_t j = 0; j < n; ++j) { std::memcpy(&pks[128 * j], keys[j].raw.data(), 128); std::memcpy(&pops[64 * j], proofs[j].raw.data(), 64); }
    check_rc("bn254_batch_pop_verify", bn254_batch_pop_verify(e.raw(), pks.data(), pops.data(), n, BN254_FLAG_REJECT_IDENTITY, status.data()));
    return status;
  }
  static void verify_possession(const PublicKey& key, const Signature& proof, Engine& e = Engine::default_engine()) {
    check_status(batch_verify_possession({key}, {proof}, e)[0]);
  }
  // register_keys with every proof checked on the device: result[j] == 0, the ErrorKind of key j, or that of its proof (9 for a wrong one) —
  // and that byte is the key's registration status: every keyed call below refuses an unproven key with it
  static std::vector<uint8_t> register_keys_proven(const std::vector<PublicKey>& keys, const std::vector<Signature>& proofs,
                                                   Engine& e = Engine::default_engine()) {
    const size_t n = keys.size();
    if (proofs.size() != n) throw Error(ErrorKind::InvalidLength);
    std::vector<uint8_t> pks(n * 128), pops(n * 64), status(n, 0);
    for (size_t j = 0; j < n; ++j) { std::memcpy(&pks[128 * j], keys[j].raw.data(), 128); std::memcpy(&pops[64 * j], proofs[j].raw.data(), 64); }
    check_rc("bn254_ctx_register_keys_pop", bn254_ctx_register_keys_pop(e.raw(), pks.data(), pops.data(), n, BN254_FLAG_REJECT_IDENTITY, status.data()));
    return status;
  }
  // result[i] == 0 iff verify(messages[i], signatures[i], registered[key_indices[i]]) succeeds; 2 (IndexOutOfBounds) outside the set
  static std::vector<uint8_t> batch_verify_keyed(const std::vector<std::vector<uint8_t>>& messages, const std::vector<Signature>& signatures,
                                                 const std::vector<uint32_t>& key_indices, Engine& e = Engine::default_engine()) {
    return verify_keyed_impl<Signature>(messages, signatures, key_indices, e);
  }
  // ... from the 33-byte wire encodings: a signature that does not decompress reads the ErrorKind Signature::from_compressed would throw (first rule)
  static std::vector<uint8_t> batch_verify_keyed(const std::vector<std::vector<uint8_t>>& messages, const std::vector<CompressedSignature>& signatures,
                                                 const std::vector<uint32_t>& key_indices, Engine& e = Engine::default_engine()) {
    return verify_keyed_impl<CompressedSignature>(messages, signatures, key_indices, e);
  }
  template <class Sig> static std::vector<uint8_t> verify_keyed_impl(const std::vector<std::vector<uint8_t>>& messages, const std::vector<Sig>& signatures,
                                                                      const std::vector<uint32_t>& key_indices, Engine& e) {
    size_t n = messages.size();
    if (signatures.size() != n || key_indices.size() != n) throw Error(ErrorKind::InvalidLength);
    const size_t sz = sizeof signatures[0].raw;
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<uint8_t> msgs, sigs(n * sz), status(n, 0);
    for (size_t i = 0; i < n; ++i) {
      off[i] = msgs.size();
      msgs.insert(msgs.end(), messages[i].begin(), messages[i].end());
      std::memcpy(&sigs[sz * i], signatures[i].raw.data(), sz);
    }
    off[n] = msgs.size();
    check_rc("bn254_batch_verify_keyed",
             bn254_batch_verify_keyed(e.raw(), msgs.data(), off.data(), sigs.data(), key_indices.data(), n, g1_input_flag<Sig>(), status.data()));
    return status;
  }
  // One message, one already aggregated signature and the indices (in the registered set of n_keys keys) of the keys that signed
  // (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap): result[i] == 0 iff e(H(m_i), sum of the named keys) * e(sigma_i, -G2) == 1;
  // 2 (IndexOutOfBounds) for an index outside the set — every such index lands on the one bit the bitmaps carry past the set.
  template <class Sig> struct SignerItemT { std::vector<uint8_t> message; Sig signature; std::vector<uint32_t> signer_indices; };
  using SignerItem = SignerItemT<Signature>;
  using CompressedSignerItem = SignerItemT<CompressedSignature>;      // the aggregate as its 33-byte wire encoding
  // the items packed as the bitmap calls take them
  struct PackedSigners { size_t bm_words; std::vector<uint64_t> off; std::vector<uint8_t> msgs, sigs; std::vector<uint32_t> bits; };
  template <class Sig> static PackedSigners pack_signers(const std::vector<SignerItemT<Sig>>& items, size_t n_keys) {
    const size_t n = items.size(), sz = std::tuple_size<decltype(Sig::raw)>::value;
    PackedSigners p{n_keys / 32 + 1, std::vector<uint64_t>(n + 1, 0), {}, std::vector<uint8_t>(n * sz), {}};
    p.bits.assign(n * p.bm_words, 0);
    for (size_t i = 0; i < n; ++i) {
      p.off[i] = p.msgs.size();
      p.msgs.insert(p.msgs.end(), items[i].message.begin(), items[i].message.end());
      std::memcpy(&p.sigs[sz * i], items[i].signature.raw.data(), sz);
      for (uint32_t j : items[i].signer_indices) {
        const size_t b = j < n_keys ? j : n_keys;
        p.bits[i * p.bm_words + b / 32] |= 1u << (b % 32);
      }
    }
    p.off[n] = p.msgs.size();
    return p;
  }
  static std::vector<uint8_t> batch_verify_keyed_signers(const std::vector<SignerItem>& items, size_t n_keys, Engine& e = Engine::default_engine()) {
    return verify_keyed_signers_impl<Signature>(items, n_keys, nullptr, 0, e);
  }
  static std::vector<uint8_t> batch_verify_keyed_signers(const std::vector<CompressedSignerItem>& items, size_t n_keys, Engine& e = Engine::default_engine()) {
    return verify_keyed_signers_impl<CompressedSignature>(items, n_keys, nullptr, 0, e);
  }
  template <class Sig> static std::vector<uint8_t> verify_keyed_signers_impl(const std::vector<SignerItemT<Sig>>& items, size_t n_keys, const uint8_t* seed32,
                                                                              uint32_t flags, Engine& e) {
    const PackedSigners p = pack_signers<Sig>(items, n_keys);
    std::vector<uint8_t> status(items.size(), 0);
    flags |= g1_input_flag<Sig>();
    if (seed32)
      check_rc("bn254_batch_verify_keyed_bitmap_randomized",
               bn254_batch_verify_keyed_bitmap_randomized(e.raw(), p.msgs.data(), p.off.data(), p.sigs.data(), p.bits.data(), p.bm_words, items.size(), flags,
                                                          seed32, status.data()));
    else
      check_rc("bn254_batch_verify_keyed_bitmap", bn254_batch_verify_keyed_bitmap(e.raw(), p.msgs.data(), p.off.data(), p.sigs.data(), p.bits.data(), p.bm_words,
                                                                                  items.size(), flags, status.data()));
    return status;
  }
  // the same through the combined checks of whole groups of items (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap_randomized): a non-zero
  // status is exact, a zero is wrong with probability <= 2^-128 per group (2^-64 with rand64) for a fresh secret seed
  static std::vector<uint8_t> batch_verify_keyed_signers_randomized(const std::vector<SignerItem>& items, size_t n_keys, const std::array<uint8_t, 32>& seed,
                                                                    bool rand64 = false, Engine& e = Engine::default_engine()) {
    return verify_keyed_signers_impl<Signature>(items, n_keys, seed.data(), rand64 ? BN254_FLAG_RAND64 : 0, e);
  }
  static std::vector<uint8_t> batch_verify_keyed_signers_randomized(const std::vector<CompressedSignerItem>& items, size_t n_keys,
                                                                    const std::array<uint8_t, 32>& seed, bool rand64 = false,
                                                                    Engine& e = Engine::default_engine()) {
    return verify_keyed_signers_impl<CompressedSignature>(items, n_keys, seed.data(), rand64 ? BN254_FLAG_RAND64 : 0, e);
  }
  static void verify_keyed_signers(const std::vector<uint8_t>& message, const Signature& signature, const std::vector<uint32_t>& signer_indices,
                                   size_t n_keys, Engine& e = Engine::default_engine()) {
    check_status(batch_verify_keyed_signers({SignerItem{message, signature, signer_indices}}, n_keys, e)[0]);
  }
  static void verify_keyed_signers(const std::vector<uint8_t>& message, const CompressedSignature& signature, const std::vector<uint32_t>& signer_indices,
                                   size_t n_keys, Engine& e = Engine::default_engine()) {
    check_status(batch_verify_keyed_signers({CompressedSignerItem{message, signature, signer_indices}}, n_keys, e)[0]);
  }
  // What a bitmap call knows besides a status (include/bn254_hip.h: bn254_batch_aggregate_keys_bitmap, bn254_batch_verify_keyed_bitmap_export,
  // bn254_ctx_set_key_weights, bn254_batch_bitmap_weights).  The bitmap rows of plain index lists, as pack_signers builds them:
  static std::vector<uint32_t> signer_bitmaps(const std::vector<std::vector<uint32_t>>& signer_lists, size_t n_keys, size_t* bm_words) {
    *bm_words = n_keys / 32 + 1;
    std::vector<uint32_t> bits(signer_lists.size() * *bm_words, 0);
    for (size_t i = 0; i < signer_lists.size(); ++i)
      for (uint32_t j : signer_lists[i]) {
        const size_t b = j < n_keys ? j : n_keys;
        bits[i * *bm_words + b / 32] |= 1u << (b % 32);
      }
    return bits;
  }
  // result[i]: status 0 and the sum of the registered keys signer_lists[i] names (the identity for an empty list or a sum that cancels), or the
  // ErrorKind of the lowest bad index (2 outside the set, else the key's registration status) and the identity
  struct AggregateKeyResult { uint8_t status; PublicKey key; };
  static std::vector<AggregateKeyResult> batch_aggregate_public_keys_signers(const std::vector<std::vector<uint32_t>>& signer_lists, size_t n_keys,
                                                                             Engine& e = Engine::default_engine()) {
    size_t bm_words = 0;
    const std::vector<uint32_t> bits = signer_bitmaps(signer_lists, n_keys, &bm_words);
    const size_t n = signer_lists.size();
    std::vector<uint8_t> keys(n * 128 + 1), status(n + 1);
    check_rc("bn254_batch_aggregate_keys_bitmap", bn254_batch_aggregate_keys_bitmap(e.raw(), bits.data(), bm_words, n, 0, keys.data(), status.data()));
    std::vector<AggregateKeyResult> out(n);
    for (size_t i = 0; i < n; ++i) { out[i].status = status[i]; std::memcpy(out[i].key.raw.data(), &keys[128 * i], 128); }
    return out;
  }
  static PublicKey aggregate_public_key_signers(const std::vector<uint32_t>& signer_indices, size_t n_keys, Engine& e = Engine::default_engine()) {
    const AggregateKeyResult r = batch_aggregate_public_keys_signers({signer_indices}, n_keys, e)[0];
    check_status(r.status);
    return r.key;
  }
  // verify_keyed_signers that also returns what the device computed: the status, H(message) and the signers' aggregate key — both zero bytes
  // unless the item passed every check before the pairing (status 0 or VerificationFailed).  Nothing is thrown for a non-zero status.
  struct ExportResult { uint8_t status; Signature hash; PublicKey key; };
  template <class Sig> static std::vector<ExportResult> verify_keyed_signers_export_impl(const std::vector<SignerItemT<Sig>>& items, size_t n_keys, Engine& e) {
    const PackedSigners p = pack_signers<Sig>(items, n_keys);
    const size_t n = items.size();
    std::vector<uint8_t> status(n + 1), hashes(n * 64 + 1), keys(n * 128 + 1);
    check_rc("bn254_batch_verify_keyed_bitmap_export",
             bn254_batch_verify_keyed_bitmap_export(e.raw(), p.msgs.data(), p.off.data(), p.sigs.data(), p.bits.data(), p.bm_words, n, g1_input_flag<Sig>(),
                                                    status.data(), hashes.data(), keys.data()));
    std::vector<ExportResult> out(n);
    for (size_t i = 0; i < n; ++i) {
      out[i].status = status[i];
      std::memcpy(out[i].hash.raw.data(), &hashes[64 * i], 64);
      std::memcpy(out[i].key.raw.data(), &keys[128 * i], 128);
    }
    return out;
  }
  static std::vector<ExportResult> batch_verify_keyed_signers_export(const std::vector<SignerItem>& items, size_t n_keys, Engine& e = Engine::default_engine()) {
    return verify_keyed_signers_export_impl<Signature>(items, n_keys, e);
  }
  static std::vector<ExportResult> batch_verify_keyed_signers_export(const std::vector<CompressedSignerItem>& items, size_t n_keys,
                                                                     Engine& e = Engine::default_engine()) {
    return verify_keyed_signers_export_impl<CompressedSignature>(items, n_keys, e);
  }
  static ExportResult verify_keyed_signers_export(const std::vector<uint8_t>& message, const Signature& signature, const std::vector<uint32_t>& signer_indices,
                                                  size_t n_keys, Engine& e = Engine::default_engine()) {
    return batch_verify_keyed_signers_export({SignerItem{message, signature, signer_indices}}, n_keys, e)[0];
  }
  static ExportResult verify_keyed_signers_export(const std::vector<uint8_t>& message, const CompressedSignature& signature,
                                                  const std::vector<uint32_t>& signer_indices, size_t n_keys, Engine& e = Engine::default_engine()) {
    return batch_verify_keyed_signers_export({CompressedSignerItem{message, signature, signer_indices}}, n_keys, e)[0];
  }
  // voting weights of the registered keys: one per key, total below 2^64 (else NativeError); every registration forgets them
  static void register_key_weights(const std::vector<uint64_t>& weights, Engine& e = Engine::default_engine()) {
    static const uint64_t none = 0;
    check_rc("bn254_ctx_set_key_weights", bn254_ctx_set_key_weights(e.raw(), weights.empty() ? &none : weights.data(), weights.size()));
  }
  static void forget_key_weights(Engine& e = Engine::default_engine()) { check_rc("bn254_ctx_set_key_weights", bn254_ctx_set_key_weights(e.raw(), nullptr, 0)); }
  // result[i]: status 0 and the sum of the weights of the keys signer_lists[i] names (a registered identity key counts), or the ErrorKind and 0
  struct WeightResult { uint8_t status; uint64_t weight; };
  static std::vector<WeightResult> batch_signers_weight(const std::vector<std::vector<uint32_t>>& signer_lists, size_t n_keys, Engine& e = Engine::default_engine()) {
    size_t bm_words = 0;
    const std::vector<uint32_t> bits = signer_bitmaps(signer_lists, n_keys, &bm_words);
    const size_t n = signer_lists.size();
    std::vector<uint64_t> weight(n + 1);
    std::vector<uint8_t> status(n + 1);
    check_rc("bn254_batch_bitmap_weights", bn254_batch_bitmap_weights(e.raw(), bits.data(), bm_words, n, weight.data(), status.data()));
    std::vector<WeightResult> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = WeightResult{status[i], weight[i]};
    return out;
  }
  static uint64_t signers_weight(const std::vector<uint32_t>& signer_indices, size_t n_keys, Engine& e = Engine::default_engine()) {
    const WeightResult r = batch_signers_weight({signer_indices}, n_keys, e)[0];
    check_status(r.status);
    return r.weight;
  }
  // The producer of such an item (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap): one message and individual signatures, signatures[k]
  // said to be by registered key key_indices[k].  Every signature is verified against its key; those that pass are added, one per key.
  // status: 0, or the message's hash ErrorKind (then nothing was added); statuses[k]: what batch_verify_keyed gives signature k.
  template <class Sig> struct ShareItemT { std::vector<uint8_t> message; std::vector<Sig> signatures; std::vector<uint32_t> key_indices; };
  using ShareItem = ShareItemT<Signature>;
  using CompressedShareItem = ShareItemT<CompressedSignature>;        // the shares as their 33-byte wire encodings; the results are the same
  struct KeyedAggregateResult { uint8_t status; Signature signature; std::vector<uint32_t> signer_indices; std::vector<uint8_t> statuses; };
  static std::vector<KeyedAggregateResult> batch_aggregate_keyed_signers(const std::vector<ShareItem>& items, size_t n_keys, Engine& e = Engine::default_engine()) {
    return aggregate_keyed_signers_impl<Signature>(items, n_keys, nullptr, 0, e);
  }
  static std::vector<KeyedAggregateResult> batch_aggregate_keyed_signers(const std::vector<CompressedShareItem>& items, size_t n_keys,
                                                                         Engine& e = Engine::default_engine()) {
    return aggregate_keyed_signers_impl<CompressedSignature>(items, n_keys, nullptr, 0, e);
  }
  // the same with ONE verify per item — the sum of its signatures that pass every check short of the pairing, against the sum of their keys —
  // and the signatures verified one by one only where that fails (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap_optimistic).  No
  // seed.  Signatures whose errors cancel within a passing item read 0 and are counted: a 0 there means "counted in a sum that verifies".
  static std::vector<KeyedAggregateResult> batch_aggregate_keyed_signers_optimistic(const std::vector<ShareItem>& items, size_t n_keys,
                                                                                    Engine& e = Engine::default_engine()) {
    return aggregate_keyed_signers_impl<Signature>(items, n_keys, nullptr, 0, e, true);
  }
  static std::vector<KeyedAggregateResult> batch_aggregate_keyed_signers_optimistic(const std::vector<CompressedShareItem>& items, size_t n_keys,
                                                                                    Engine& e = Engine::default_engine()) {
    return aggregate_keyed_signers_impl<CompressedSignature>(items, n_keys, nullptr, 0, e, true);
  }
  // the same through the combined checks of 64 signatures of one key at a time, across the items of the call (include/bn254_hip.h:
  // bn254_batch_collect_keyed_bitmap_randomized): the same results; a non-zero status is exact, a zero is wrong with probability <= 2^-128 per
  // group (2^-64 with rand64) for a fresh SECRET seed
  static std::vector<KeyedAggregateResult> batch_aggregate_keyed_signers_randomized(const std::vector<ShareItem>& items, size_t n_keys,
                                                                                    const std::array<uint8_t, 32>& seed, bool rand64 = false,
                                                                                    Engine& e = Engine::default_engine()) {
    return aggregate_keyed_signers_impl<Signature>(items, n_keys, seed.data(), rand64 ? BN254_FLAG_RAND64 : 0, e);
  }
  static std::vector<KeyedAggregateResult> batch_aggregate_keyed_signers_randomized(const std::vector<CompressedShareItem>& items, size_t n_keys,
                                                                                    const std::array<uint8_t, 32>& seed, bool rand64 = false,
                                                                                    Engine& e = Engine::default_engine()) {
    return aggregate_keyed_signers_impl<CompressedSignature>(items, n_keys, seed.data(), rand64 ? BN254_FLAG_RAND64 : 0, e);
  }
  template <class Sig> static std::vector<KeyedAggregateResult> aggregate_keyed_signers_impl(const std::vector<ShareItemT<Sig>>& items, size_t n_keys,
                                                                                             const uint8_t* seed32, uint32_t flags, Engine& e,
                                                                                             bool optimistic = false) {
    flags |= g1_input_flag<Sig>();
    const size_t n = items.size(), bm_words = (n_keys + 31) / 32 ? (n_keys + 31) / 32 : 1;
    std::vector<uint64_t> off(n + 1, 0), share_off(n + 1, 0);
    std::vector<uint8_t> msgs, shares;
    std::vector<uint32_t> keys;
    for (size_t i = 0; i < n; ++i) {
      if (items[i].signatures.size() != items[i].key_indices.size()) throw Error(ErrorKind::InvalidLength);
      off[i] = msgs.size();
      share_off[i] = keys.size();
      msgs.insert(msgs.end(), items[i].message.begin(), items[i].message.end());
      for (const Sig& s : items[i].signatures) shares.insert(shares.end(), s.raw.begin(), s.raw.end());
      keys.insert(keys.end(), items[i].key_indices.begin(), items[i].key_indices.end());
    }
    off[n] = msgs.size();
    share_off[n] = keys.size();
    std::vector<uint8_t> share_st(keys.size() + 1, 0), tuple_st(n + 1, 0), agg(n * 64 + 1, 0);
    std::vector<uint32_t> bits(n * bm_words + 1, 0);
    shares.resize(shares.size() + 1);
    keys.resize(keys.size() + 1);
    if (optimistic)
      check_rc("bn254_batch_collect_keyed_bitmap_optimistic",
               bn254_batch_collect_keyed_bitmap_optimistic(e.raw(), msgs.data(), off.data(), shares.data(), keys.data(), share_off.data(), share_off[n], n,
                                                           bm_words, flags, share_st.data(), tuple_st.data(), agg.data(), bits.data(), nullptr));
    else if (seed32)
      check_rc("bn254_batch_collect_keyed_bitmap_randomized",
               bn254_batch_collect_keyed_bitmap_randomized(e.raw(), msgs.data(), off.data(), shares.data(), keys.data(), share_off.data(), share_off[n], n,
                                                           bm_words, flags, seed32, share_st.data(), tuple_st.data(), agg.data(), bits.data(), nullptr));
    else
      check_rc("bn254_batch_collect_keyed_bitmap",
               bn254_batch_collect_keyed_bitmap(e.raw(), msgs.data(), off.data(), shares.data(), keys.data(), share_off.data(), share_off[n], n, bm_words, flags,
                                                share_st.data(), tuple_st.data(), agg.data(), bits.data(), nullptr));
    std::vector<KeyedAggregateResult> out(n);
    for (size_t i = 0; i < n; ++i) {
      out[i].status = tuple_st[i];
      std::memcpy(out[i].signature.raw.data(), &agg[64 * i], 64);
      for (size_t j = 0; j < 32 * bm_words; ++j)
        if ((bits[i * bm_words + j / 32] >> (j % 32)) & 1u) out[i].signer_indices.push_back((uint32_t)j);
      out[i].statuses.assign(share_st.begin() + share_off[i], share_st.begin() + share_off[i + 1]);
    }
    return out;
  }
  static KeyedAggregateResult aggregate_keyed_signers(const std::vector<uint8_t>& message, const std::vector<Signature>& signatures,
                                                      const std::vector<uint32_t>& key_indices, size_t n_keys, Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = batch_aggregate_keyed_signers({ShareItem{message, signatures, key_indices}}, n_keys, e)[0];
    check_status(r.status);
    return r;
  }
  static KeyedAggregateResult aggregate_keyed_signers(const std::vector<uint8_t>& message, const std::vector<CompressedSignature>& signatures,
                                                      const std::vector<uint32_t>& key_indices, size_t n_keys, Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = batch_aggregate_keyed_signers({CompressedShareItem{message, signatures, key_indices}}, n_keys, e)[0];
    check_status(r.status);
    return r;
  }
  static KeyedAggregateResult aggregate_keyed_signers_optimistic(const std::vector<uint8_t>& message, const std::vector<Signature>& signatures,
                                                                 const std::vector<uint32_t>& key_indices, size_t n_keys,
                                                                 Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = batch_aggregate_keyed_signers_optimistic({ShareItem{message, signatures, key_indices}}, n_keys, e)[0];
    check_status(r.status);
    return r;
  }
  static KeyedAggregateResult aggregate_keyed_signers_randomized(const std::vector<uint8_t>& message, const std::vector<Signature>& signatures,
                                                                 const std::vector<uint32_t>& key_indices, size_t n_keys, const std::array<uint8_t, 32>& seed,
                                                                 bool rand64 = false, Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = batch_aggregate_keyed_signers_randomized({ShareItem{message, signatures, key_indices}}, n_keys, seed, rand64, e)[0];
    check_status(r.status);
    return r;
  }
  // t-of-n threshold signatures over the registered keys (include/bn254_hip.h: bn254_batch_threshold_combine_keyed): registered key j is the
  // share key f(j + 1) * G2 of a dealing, an item's signatures are the validators' shares.  Every share is verified against its key; with at
  // least `threshold` keys holding a valid share, the shares of the `threshold` lowest such keys are interpolated at zero: `signature` is the
  // group signature (verify accepts it under f(0) * G2) and signer_indices the keys used.  status 9 (VerificationFailed): too few valid keys —
  // signer_indices then lists who was there and the signature is the identity; else the message's hash ErrorKind.  That the registered keys
  // lie on one polynomial of degree threshold - 1 is check_dealing's to check, once per key set.
  static std::vector<KeyedAggregateResult> batch_threshold_combine_keyed(const std::vector<ShareItem>& items, size_t n_keys, uint32_t threshold,
                                                                         Engine& e = Engine::default_engine()) {
    return threshold_batch<Signature>(items, n_keys, threshold, false, e);
  }
  static std::vector<KeyedAggregateResult> batch_threshold_combine_keyed(const std::vector<CompressedShareItem>& items, size_t n_keys, uint32_t threshold,
                                                                         Engine& e = Engine::default_engine()) {
    return threshold_batch<CompressedSignature>(items, n_keys, threshold, false, e);
  }
  // THE GROUP KEY f(0) * G2 of the registered dealing, for the optimistic calls below (include/bn254_hip.h: bn254_ctx_set_group_key); throws
  // the key's decode Error, and then no group key is set.  forget_group_key drops it, as register_keys / register_keys_proven do: a new key
  // set is a new dealing.  This call does not check that the registered keys interpolate to this key: check_dealing computes the key they do.
  static void register_group_key(const PublicKey& group_key, Engine& e = Engine::default_engine()) {
    uint8_t st = 0;
    check_rc("bn254_ctx_set_group_key", bn254_ctx_set_group_key(e.raw(), group_key.raw.data(), 0, &st));
    check_status(st);
  }
  static void forget_group_key(Engine& e = Engine::default_engine()) {
    check_rc("bn254_ctx_set_group_key", bn254_ctx_set_group_key(e.raw(), nullptr, 0, nullptr));
  }
  // batch_threshold_combine_keyed by interpolating the `threshold` lowest keys with a well-formed share first and verifying the RESULT once
  // under the group key (include/bn254_hip.h: bn254_batch_threshold_combine_keyed_optimistic).  A result that passes is the group signature;
  // the shares outside the keys used were then not verified (status 0 if well-formed and naming a registered key), and shares whose errors
  // cancel under the coefficients read 0.  A result that fails sends the item through the exact call: the same result.  Without a group
  // key the call is refused (bad argument).
  static std::vector<KeyedAggregateResult> batch_threshold_combine_keyed_optimistic(const std::vector<ShareItem>& items, size_t n_keys, uint32_t threshold,
                                                                                    Engine& e = Engine::default_engine()) {
    return threshold_batch<Signature>(items, n_keys, threshold, true, e);
  }
  static std::vector<KeyedAggregateResult> batch_threshold_combine_keyed_optimistic(const std::vector<CompressedShareItem>& items, size_t n_keys,
                                                                                    uint32_t threshold, Engine& e = Engine::default_engine()) {
    return threshold_batch<CompressedSignature>(items, n_keys, threshold, true, e);
  }
  static KeyedAggregateResult threshold_combine_keyed_optimistic(const std::vector<uint8_t>& message, const std::vector<Signature>& signatures,
                                                                 const std::vector<uint32_t>& key_indices, size_t n_keys, uint32_t threshold,
                                                                 Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = threshold_batch<Signature>({ShareItem{message, signatures, key_indices}}, n_keys, threshold, true, e)[0];
    check_status(r.status);
    return r;
  }
  template <class Sig> static std::vector<KeyedAggregateResult> threshold_batch(const std::vector<ShareItemT<Sig>>& items, size_t n_keys, uint32_t threshold,
                                                                                bool optimistic, Engine& e) {
    if (threshold == 0) throw Error(ErrorKind::InvalidLength);
    const uint32_t flags = g1_input_flag<Sig>();
    const size_t n = items.size(), bm_words = (n_keys + 31) / 32 ? (n_keys + 31) / 32 : 1;
    std::vector<uint64_t> off(n + 1, 0), share_off(n + 1, 0);
    std::vector<uint8_t> msgs, shares;
    std::vector<uint32_t> keys;
    for (size_t i = 0; i < n; ++i) {
      if (items[i].signatures.size() != items[i].key_indices.size()) throw Error(ErrorKind::InvalidLength);
      off[i] = msgs.size();
      share_off[i] = keys.size();
      msgs.insert(msgs.end(), items[i].message.begin(), items[i].message.end());
      for (const Sig& s : items[i].signatures) shares.insert(shares.end(), s.raw.begin(), s.raw.end());
      keys.insert(keys.end(), items[i].key_indices.begin(), items[i].key_indices.end());
    }
    off[n] = msgs.size();
    share_off[n] = keys.size();
    std::vector<uint8_t> share_st(keys.size() + 1, 0), tuple_st(n + 1, 0), group(n * 64 + 1, 0);
    std::vector<uint32_t> bits(n * bm_words + 1, 0);
    shares.resize(shares.size() + 1);
    keys.resize(keys.size() + 1);
    if (optimistic)
      check_rc("bn254_batch_threshold_combine_keyed_optimistic",
               bn254_batch_threshold_combine_keyed_optimistic(e.raw(), msgs.data(), off.data(), shares.data(), keys.data(), share_off.data(), share_off[n], n,
                                                              bm_words, threshold, flags, share_st.data(), tuple_st.data(), group.data(), bits.data(), nullptr));
    else
      check_rc("bn254_batch_threshold_combine_keyed",
               bn254_batch_threshold_combine_keyed(e.raw(), msgs.data(), off.data(), shares.data(), keys.data(), share_off.data(), share_off[n], n, bm_words,
                                                   threshold, flags, share_st.data(), tuple_st.data(), group.data(), bits.data(), nullptr));
    std::vector<KeyedAggregateResult> out(n);
    for (size_t i = 0; i < n; ++i) {
      out[i].status = tuple_st[i];
      std::memcpy(out[i].signature.raw.data(), &group[64 * i], 64);
      for (size_t j = 0; j < 32 * bm_words; ++j)
        if ((bits[i * bm_words + j / 32] >> (j % 32)) & 1u) out[i].signer_indices.push_back((uint32_t)j);
      out[i].statuses.assign(share_st.begin() + share_off[i], share_st.begin() + share_off[i + 1]);
    }
    return out;
  }
  static KeyedAggregateResult threshold_combine_keyed(const std::vector<uint8_t>& message, const std::vector<Signature>& signatures,
                                                      const std::vector<uint32_t>& key_indices, size_t n_keys, uint32_t threshold,
                                                      Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = batch_threshold_combine_keyed({ShareItem{message, signatures, key_indices}}, n_keys, threshold, e)[0];
    check_status(r.status);
    return r;
  }
  static KeyedAggregateResult threshold_combine_keyed(const std::vector<uint8_t>& message, const std::vector<CompressedSignature>& signatures,
                                                      const std::vector<uint32_t>& key_indices, size_t n_keys, uint32_t threshold,
                                                      Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = batch_threshold_combine_keyed({CompressedShareItem{message, signatures, key_indices}}, n_keys, threshold, e)[0];
    check_status(r.status);
    return r;
  }
  static KeyedAggregateResult threshold_combine_keyed_optimistic(const std::vector<uint8_t>& message, const std::vector<CompressedSignature>& signatures,
                                                                 const std::vector<uint32_t>& key_indices, size_t n_keys, uint32_t threshold,
                                                                 Engine& e = Engine::default_engine()) {
    KeyedAggregateResult r = threshold_batch<CompressedSignature>({CompressedShareItem{message, signatures, key_indices}}, n_keys, threshold, true, e)[0];
    check_status(r.status);
    return r;
  }
  // sum scalars[k] * points[k] in G1 (include/bn254_hip.h: bn254_batch_g1_msm), scalars as 32 big-endian bytes each, taken mod r
  static Signature g1_msm(const std::vector<Signature>& points, const std::vector<std::array<uint8_t, 32>>& scalars, Engine& e = Engine::default_engine()) {
    if (points.size() != scalars.size()) throw Error(ErrorKind::InvalidLength);
    std::vector<uint8_t> p(points.size() * 64 + 4, 0), k(points.size() * 32 + 4, 0);
    for (size_t i = 0; i < points.size(); ++i) {
      std::memcpy(&p[64 * i], points[i].raw.data(), 64);
      std::memcpy(&k[32 * i], scalars[i].data(), 32);
    }
    const uint64_t seg[2] = {0, points.size()};
    Signature out;
    uint8_t st = 0;
    check_rc("bn254_batch_g1_msm", bn254_batch_g1_msm(e.raw(), p.data(), k.data(), seg, 1, 1, out.raw.data(), &st));
    check_status(st);
    return out;
  }
  // ... and in G2 (include/bn254_hip.h: bn254_batch_g2_msm): group keys, sum x^k C_k over a vector of commitments
  static PublicKey g2_msm(const std::vector<PublicKey>& points, const std::vector<std::array<uint8_t, 32>>& scalars, Engine& e = Engine::default_engine()) {
    if (points.size() != scalars.size()) throw Error(ErrorKind::InvalidLength);
    std::vector<uint8_t> p(points.size() * 128 + 4, 0), k(points.size() * 32 + 4, 0);
    for (size_t i = 0; i < points.size(); ++i) {
      std::memcpy(&p[128 * i], points[i].raw.data(), 128);
      std::memcpy(&k[32 * i], scalars[i].data(), 32);
    }
    const uint64_t seg[2] = {0, points.size()};
    PublicKey out;
    uint8_t st = 0;
    check_rc("bn254_batch_g2_msm", bn254_batch_g2_msm(e.raw(), p.data(), k.data(), seg, 1, 1, out.raw.data(), &st));
    check_status(st);
    return out;
  }
  // Are the registered keys (key j standing for x_j = j + 1) a `threshold`-of-n dealing — do they lie on one polynomial of degree below
  // `threshold` (include/bn254_hip.h: bn254_ctx_check_dealing)?  Returns the group key they interpolate to and, with register_key, names it
  // as the group key of the optimistic calls.  Throws Error(VerificationFailed) for a key set that is no dealing, and the Error of the lowest
  // key whose registration status is non-zero, its index then in *bad_key (UINT32_MAX otherwise).  Randomised over the seed: a refusal is
  // always right, an acceptance wrong with probability at most 2^-128 for a fresh seed — drawn after the keys were fixed — and keys
  // registered with the subgroup check (register_keys always runs it).
  static PublicKey check_dealing(uint32_t threshold, const std::array<uint8_t, 32>& seed, bool register_key = false, uint32_t* bad_key = nullptr,
                                 Engine& e = Engine::default_engine()) {
    PublicKey key;
    uint8_t st = 0;
    uint32_t bad = UINT32_MAX;
    check_rc("bn254_ctx_check_dealing", bn254_ctx_check_dealing(e.raw(), threshold, seed.data(), 0, key.raw.data(), &st, &bad));
    if (bad_key) *bad_key = bad;
    check_status(st);
    if (register_key) register_group_key(key, e);
    return key;
  }
  // VECTORS OF G2 POINTS combined column by column, one scalar per vector (include/bn254_hip.h: bn254_batch_g2_vector_combine):
  // result[k] = sum_i scalars[i] * vectors[i][k], the scalars 32 big-endian bytes reduced mod r; throws the first decode Error
  static std::vector<PublicKey> g2_vector_combine(const std::vector<std::vector<PublicKey>>& vectors, const std::vector<std::array<uint8_t, 32>>& scalars,
                                                  Engine& e = Engine::default_engine()) {
    if (vectors.empty() || vectors[0].empty() || vectors.size() != scalars.size()) throw Error(ErrorKind::InvalidLength);
    const size_t d = vectors.size(), len = vectors[0].size();
    std::vector<uint8_t> v(d * len * 128), k(d * 32), out(len * 128), st(len, 0);
    for (size_t i = 0; i < d; ++i) {
      if (vectors[i].size() != len) throw Error(ErrorKind::InvalidLength);
      for (size_t j = 0; j < len; ++j) std::memcpy(&v[128 * (i * len + j)], vectors[i][j].raw.data(), 128);
      std::memcpy(&k[32 * i], scalars[i].data(), 32);
    }
    check_rc("bn254_batch_g2_vector_combine", bn254_batch_g2_vector_combine(e.raw(), v.data(), k.data(), d, len, 1, out.data(), st.data()));
    std::vector<PublicKey> sum(len);
    for (size_t j = 0; j < len; ++j) {
      check_status(st[j]);
      std::memcpy(sum[j].raw.data(), &out[128 * j], 128);
    }
    return sum;
  }
  // RESHARE (include/bn254_hip.h: bn254_ctx_reshare_commitments): hand the registered (OLD) committee's group key on to the next committee.
  // dealers: (key index, that old member's commitments to its sub-dealing — t_new of them, the first its registered key), sorted here by
  // index; a repeated index throws std::invalid_argument.  n_keys: the size of the registered set.  The `threshold` lowest qualified
  // indices are combined under their Lagrange coefficients: commitments[0] is the unchanged group key, and register_keys_from_commitments
  // registers the new committee from `commitments`.  Too few qualified dealers: throws ReshareFailed.  Not checked: that the registered keys
  // are a dealing (check_dealing), that the private sub-shares match the vectors (each recipient's batch_verify_dealt_shares).
  struct Reshare {
    std::vector<PublicKey> commitments;
    std::vector<uint32_t> used;          // S: the key indices combined, increasing
    std::vector<uint8_t> statuses;       // per dealer in index order: 0 or its ErrorKind
  };
  static Reshare reshare_commitments(std::vector<std::pair<uint32_t, std::vector<PublicKey>>> dealers, uint32_t threshold, size_t n_keys,
                                     Engine& e = Engine::default_engine()) {
    if (dealers.empty() || dealers[0].second.empty() || n_keys == 0) throw Error(ErrorKind::InvalidLength);
    std::sort(dealers.begin(), dealers.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    const size_t d = dealers.size(), t_new = dealers[0].second.size(), bm_words = (n_keys + 31) / 32;
    std::vector<uint8_t> v(d * t_new * 128), out(t_new * 128), st(d, 0);
    std::vector<uint32_t> keys(d), row(bm_words, 0);
    for (size_t i = 0; i < d; ++i) {
      if (dealers[i].second.size() != t_new) throw Error(ErrorKind::InvalidLength);
      if (i && dealers[i].first == dealers[i - 1].first) throw std::invalid_argument("a dealer index is repeated");
      keys[i] = dealers[i].first;
      for (size_t k = 0; k < t_new; ++k) std::memcpy(&v[128 * (i * t_new + k)], dealers[i].second[k].raw.data(), 128);
    }
    uint8_t status = 0;
    check_rc("bn254_ctx_reshare_commitments", bn254_ctx_reshare_commitments(e.raw(), v.data(), keys.data(), d, (uint32_t)t_new, threshold, 0, st.data(),
                                                                            row.data(), bm_words, out.data(), &status));
    Reshare r;
    for (size_t w = 0; w < bm_words; ++w)
      for (uint32_t b = 0; b < 32; ++b)
        if ((row[w] >> b) & 1u) r.used.push_back((uint32_t)(32 * w + b));
    if (status != 0) throw ReshareFailed(st, r.used);
    r.statuses = st;
    r.commitments.resize(t_new);
    for (size_t k = 0; k < t_new; ++k) std::memcpy(r.commitments[k].raw.data(), &out[128 * k], 128);
    return r;
  }
  // FELDMAN COMMITMENTS (include/bn254_hip.h: bn254_batch_g2_poly_eval, bn254_ctx_register_keys_commitments).  A dealer publishes the
  // commitments C_k = a_k * G2 of its polynomial, lowest degree first; the share key of key index j is their value at x = j + 1.
  // commitments_eval: the polynomial with these coefficients at each of xs, sum x^k C_k; throws the first commitment's decode Error.
  static std::vector<PublicKey> commitments_eval(const std::vector<PublicKey>& commitments, const std::vector<uint32_t>& xs,
                                                 Engine& e = Engine::default_engine()) {
    const size_t t = commitments.size(), q = xs.size();
    std::vector<uint8_t> c(t * 128 + 4, 0), out(q * 128 + 4, 0), st(q + 1, 0);
    for (size_t k = 0; k < t; ++k) std::memcpy(&c[128 * k], commitments[k].raw.data(), 128);
    const uint64_t off[2] = {0, t};
    const std::vector<uint32_t> poly(q + 1, 0);
    check_rc("bn254_batch_g2_poly_eval", bn254_batch_g2_poly_eval(e.raw(), c.data(), off, 1, poly.data(), xs.data(), q, out.data(), st.data()));
    std::vector<PublicKey> values(q);
    for (size_t i = 0; i < q; ++i) {
      check_status(st[i]);
      std::memcpy(values[i].raw.data(), &out[128 * i], 128);
    }
    return values;
  }
  // register the n share keys of the dealing these commitments belong to, derived on the device: register_keys on
  // commitments_eval(commitments, 1 .. n) without the keys crossing to the host and back.  result[j] == 0 or the ErrorKind of key j; a
  // commitment that does not decode throws its Error, and then NO keys are registered.  register_key: commitments[0] is then named as the
  // group key (register_group_key, whose checks apply).  check_dealing(commitments.size(), seed) passes on such a set by construction.
  static std::vector<uint8_t> register_keys_from_commitments(const std::vector<PublicKey>& commitments, size_t n, bool register_key = false,
                                                             Engine& e = Engine::default_engine()) {
    if (commitments.empty() || n == 0) throw Error(ErrorKind::InvalidLength);
    std::vector<uint8_t> c(commitments.size() * 128), key_status(n, 0);
    for (size_t k = 0; k < commitments.size(); ++k) std::memcpy(&c[128 * k], commitments[k].raw.data(), 128);
    uint8_t st = 0;
    check_rc("bn254_ctx_register_keys_commitments",
             bn254_ctx_register_keys_commitments(e.raw(), c.data(), (uint32_t)commitments.size(), n, 0, key_status.data(), &st));
    check_status(st);
    if (register_key) register_group_key(commitments[0], e);
    return key_status;
  }
  // the commitments of the SUM of the qualified dealers' polynomials: the element-wise sum of their vectors, all of one length
  static std::vector<PublicKey> combine_commitments(const std::vector<std::vector<PublicKey>>& vectors, Engine& e = Engine::default_engine()) {
    if (vectors.empty() || vectors[0].empty()) throw Error(ErrorKind::InvalidLength);
    const size_t d = vectors.size(), t = vectors[0].size();
    std::vector<uint8_t> pts(d * t * 128), out(t * 128), st(t, 0);
    std::vector<uint64_t> seg(t + 1);
    for (size_t k = 0; k <= t; ++k) seg[k] = k * d;
    for (size_t i = 0; i < d; ++i) {
      if (vectors[i].size() != t) throw Error(ErrorKind::InvalidLength);
      for (size_t k = 0; k < t; ++k) std::memcpy(&pts[128 * (k * d + i)], vectors[i][k].raw.data(), 128);
    }
    check_rc("bn254_batch_g2_sum", bn254_batch_g2_sum(e.raw(), pts.data(), seg.data(), t, out.data(), st.data()));
    std::vector<PublicKey> sum(t);
    for (size_t k = 0; k < t; ++k) {
      check_status(st[k]);
      std::memcpy(sum[k].raw.data(), &out[128 * k], 128);
    }
    return sum;
  }
  // what the holder of key `index` checks in a DKG round: result[d] == 0 iff secrets[d] * G2::one() equals dealer d's vector at index + 1,
  // 9 (VerificationFailed) if not, else the decode ErrorKind of that dealer's first faulty commitment
  static std::vector<uint8_t> batch_verify_dealt_shares(const std::vector<std::vector<PublicKey>>& vectors, uint32_t index,
                                                        const std::vector<PrivateKey>& secrets, Engine& e = Engine::default_engine()) {
    const size_t d = vectors.size();
    if (secrets.size() != d || index == UINT32_MAX) throw Error(ErrorKind::InvalidLength);
    std::vector<uint64_t> off(d + 1, 0);
    for (size_t i = 0; i < d; ++i) off[i + 1] = off[i] + vectors[i].size();
    std::vector<uint8_t> c(off[d] * 128 + 4, 0), right(d * 128 + 4, 0), st(d + 1, 0);
    std::vector<uint32_t> poly(d + 1, 0), xs(d + 1, index + 1);
    for (size_t i = 0; i < d; ++i) {
      poly[i] = (uint32_t)i;
      for (size_t k = 0; k < vectors[i].size(); ++k) std::memcpy(&c[128 * (off[i] + k)], vectors[i][k].raw.data(), 128);
    }
    check_rc("bn254_batch_g2_poly_eval", bn254_batch_g2_poly_eval(e.raw(), c.data(), off.data(), d, poly.data(), xs.data(), d, right.data(), st.data()));
    std::vector<uint8_t> verdict(d, 0);
    for (size_t i = 0; i < d; ++i) {
      const PublicKey left = PublicKey::from_private_key(secrets[i], e);
      verdict[i] = st[i] ? st[i] : std::memcmp(left.raw.data(), &right[128 * i], 128) == 0 ? 0 : (uint8_t)ErrorKind::VerificationFailed;
    }
    return verdict;
  }
  // The inner node of an aggregation tree (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap): one message and PARTIAL aggregates of it,
  // parts[k] = a summed signature and the indices of the registered keys it is said to sum.  Every partial is verified as verify_keyed_signers
  // verifies it; in the order given, the valid ones whose indices do not overlap what was taken before are added (first fit).
  // status: 0, or the message's hash ErrorKind (then nothing was added); statuses[k]: what verify_keyed_signers gives partial k; taken[k]: 1 or 0.
  template <class Sig> struct PartialAggregateT { Sig signature; std::vector<uint32_t> signer_indices; };
  template <class Sig> struct MergeItemT { std::vector<uint8_t> message; std::vector<PartialAggregateT<Sig>> parts; };
  using PartialAggregate = PartialAggregateT<Signature>;
  using MergeItem = MergeItemT<Signature>;
  using CompressedPartialAggregate = PartialAggregateT<CompressedSignature>;     // the partials as their 33-byte wire encodings
  using CompressedMergeItem = MergeItemT<CompressedSignature>;
  struct KeyedMergeResult { uint8_t status; Signature signature; std::vector<uint32_t> signer_indices; std::vector<uint8_t> statuses, taken; };
  static std::vector<KeyedMergeResult> batch_merge_keyed_signers(const std::vector<MergeItem>& items, size_t n_keys, Engine& e = Engine::default_engine(),
                                                                 bool optimistic = false) {
    return merge_keyed_signers_impl<Signature>(items, n_keys, e, optimistic);
  }
  static std::vector<KeyedMergeResult> batch_merge_keyed_signers(const std::vector<CompressedMergeItem>& items, size_t n_keys,
                                                                 Engine& e = Engine::default_engine(), bool optimistic = false) {
    return merge_keyed_signers_impl<CompressedSignature>(items, n_keys, e, optimistic);
  }
  template <class Sig> static std::vector<KeyedMergeResult> merge_keyed_signers_impl(const std::vector<MergeItemT<Sig>>& items, size_t n_keys, Engine& e,
                                                                                     bool optimistic) {
    const size_t n = items.size(), bm_words = n_keys / 32 + 1;   // one bit past the set: every index outside it lands there -> IndexOutOfBounds
    const size_t sz = std::tuple_size<decltype(Sig::raw)>::value;
    const uint32_t flags = g1_input_flag<Sig>();
    std::vector<uint64_t> off(n + 1, 0), part_off(n + 1, 0);
    std::vector<uint8_t> msgs, parts;
    std::vector<uint32_t> rows;
    for (size_t i = 0; i < n; ++i) {
      off[i] = msgs.size();
      part_off[i] = parts.size() / sz;
      msgs.insert(msgs.end(), items[i].message.begin(), items[i].message.end());
      for (const PartialAggregateT<Sig>& p : items[i].parts) {
        parts.insert(parts.end(), p.signature.raw.begin(), p.signature.raw.end());
        rows.resize(rows.size() + bm_words, 0);
        for (uint32_t j : p.signer_indices) {
          const size_t b = j < n_keys ? j : n_keys;
          rows[rows.size() - bm_words + b / 32] |= 1u << (b % 32);
        }
      }
    }
    off[n] = msgs.size();
    part_off[n] = parts.size() / sz;
    const size_t n_parts = (size_t)part_off[n];
    std::vector<uint8_t> part_st(n_parts + 1, 0), taken(n_parts + 1, 0), tuple_st(n + 1, 0), agg(n * 64 + 1, 0);
    std::vector<uint32_t> bits(n * bm_words + 1, 0);
    parts.resize(parts.size() + 1);
    rows.resize(rows.size() + 1);
    if (optimistic)
      check_rc("bn254_batch_merge_keyed_bitmap_optimistic",
               bn254_batch_merge_keyed_bitmap_optimistic(e.raw(), msgs.data(), off.data(), parts.data(), rows.data(), part_off.data(), n_parts, n, bm_words, flags,
                                                         part_st.data(), taken.data(), tuple_st.data(), agg.data(), bits.data(), nullptr));
    else
      check_rc("bn254_batch_merge_keyed_bitmap",
               bn254_batch_merge_keyed_bitmap(e.raw(), msgs.data(), off.data(), parts.data(), rows.data(), part_off.data(), n_parts, n, bm_words, flags, part_st.data(),
                                              taken.data(), tuple_st.data(), agg.data(), bits.data(), nullptr));
    std::vector<KeyedMergeResult> out(n);
    for (size_t i = 0; i < n; ++i) {
      out[i].status = tuple_st[i];
      std::memcpy(out[i].signature.raw.data(), &agg[64 * i], 64);
      for (size_t j = 0; j < 32 * bm_words; ++j)
        if ((bits[i * bm_words + j / 32] >> (j % 32)) & 1u) out[i].signer_indices.push_back((uint32_t)j);
      out[i].statuses.assign(part_st.begin() + part_off[i], part_st.begin() + part_off[i + 1]);
      out[i].taken.assign(taken.begin() + part_off[i], taken.begin() + part_off[i + 1]);
    }
    return out;
  }
  static KeyedMergeResult merge_keyed_signers(const std::vector<uint8_t>& message, const std::vector<PartialAggregate>& parts, size_t n_keys,
                                              Engine& e = Engine::default_engine()) {
    KeyedMergeResult r = batch_merge_keyed_signers({MergeItem{message, parts}}, n_keys, e)[0];
    check_status(r.status);
    return r;
  }
  static KeyedMergeResult merge_keyed_signers(const std::vector<uint8_t>& message, const std::vector<CompressedPartialAggregate>& parts, size_t n_keys,
                                              Engine& e = Engine::default_engine()) {
    KeyedMergeResult r = batch_merge_keyed_signers({CompressedMergeItem{message, parts}}, n_keys, e)[0];
    check_status(r.status);
    return r;
  }
  // ... with ONE verify per item — the sum of its partials that pass every check short of the pairing, against the keys of the union of their
  // indices — and the partials verified one by one only where that fails or two of them overlap (include/bn254_hip.h:
  // bn254_batch_merge_keyed_bitmap_optimistic).  The same results, with one deviation: partials whose errors cancel within an item that passes
  // read 0 and are taken; the aggregate is still the valid one for the union.  Who needs per-partial verdicts takes batch_merge_keyed_signers.
  static std::vector<KeyedMergeResult> batch_merge_keyed_signers_optimistic(const std::vector<MergeItem>& items, size_t n_keys,
                                                                            Engine& e = Engine::default_engine()) {
    return batch_merge_keyed_signers(items, n_keys, e, true);
  }
  static std::vector<KeyedMergeResult> batch_merge_keyed_signers_optimistic(const std::vector<CompressedMergeItem>& items, size_t n_keys,
                                                                            Engine& e = Engine::default_engine()) {
    return batch_merge_keyed_signers(items, n_keys, e, true);
  }
  static KeyedMergeResult merge_keyed_signers_optimistic(const std::vector<uint8_t>& message, const std::vector<PartialAggregate>& parts, size_t n_keys,
                                                         Engine& e = Engine::default_engine()) {
    KeyedMergeResult r = batch_merge_keyed_signers_optimistic({MergeItem{message, parts}}, n_keys, e)[0];
    check_status(r.status);
    return r;
  }
  // aggregate_verify against the registered set: key_indices[j] names the key of messages[j]; 2 (IndexOutOfBounds) outside the set
  // (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed)
  struct KeyedAggregate { std::vector<std::vector<uint8_t>> messages; Signature signature; std::vector<uint32_t> key_indices; };
  static void aggregate_verify_keyed(const std::vector<std::vector<uint8_t>>& messages, const Signature& signature, const std::vector<uint32_t>& key_indices,
                                     Engine& e = Engine::default_engine()) {
    check_status(batch_aggregate_verify_distinct_keyed({KeyedAggregate{messages, signature, key_indices}}, e)[0]);
  }
  // result[i] == 0 iff aggregate_verify_keyed on aggregates[i] succeeds, else the ErrorKind it would throw
  static std::vector<uint8_t> batch_aggregate_verify_distinct_keyed(const std::vector<KeyedAggregate>& aggregates, Engine& e = Engine::default_engine()) {
    return keyed_aggregates(aggregates, nullptr, 0, e);
  }
  // opt-in randomised mode (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed_randomized): the same result shape; non-zero
  // entries are exact, a zero is wrong with probability <= 2^-128 per group (2^-64 with rand64) for a fresh secret 32-byte seed
  static std::vector<uint8_t> batch_aggregate_verify_distinct_keyed_randomized(const std::vector<KeyedAggregate>& aggregates,
                                                                              const std::array<uint8_t, 32>& seed, Engine& e = Engine::default_engine(),
                                                                              bool rand64 = false) {
    return keyed_aggregates(aggregates, seed.data(), rand64 ? BN254_FLAG_RAND64 : 0, e);
  }
  // the two keyed aggregate calls: seed == nullptr the exact one, else the randomised one with these flags
  static std::vector<uint8_t> keyed_aggregates(const std::vector<KeyedAggregate>& aggregates, const uint8_t* seed, uint32_t flags, Engine& e) {
    const size_t n = aggregates.size();
    std::vector<uint64_t> msg_off(1, 0), agg_off(1, 0);
    std::vector<uint32_t> idx;
    std::vector<uint8_t> msgs, sigs(n * 64), status(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const KeyedAggregate& a = aggregates[i];
      if (a.messages.size() != a.key_indices.size()) throw Error(ErrorKind::InvalidLength);
      for (size_t j = 0; j < a.messages.size(); ++j) {
        msgs.insert(msgs.end(), a.messages[j].begin(), a.messages[j].end());
        msg_off.push_back(msgs.size());
      }
      idx.insert(idx.end(), a.key_indices.begin(), a.key_indices.end());
      agg_off.push_back(msg_off.size() - 1);
      std::memcpy(&sigs[64 * i], a.signature.raw.data(), 64);
    }
    const size_t m = msg_off.size() - 1;
    if (seed)
      check_rc("bn254_batch_aggregate_verify_distinct_keyed_randomized",
               bn254_batch_aggregate_verify_distinct_keyed_randomized(e.raw(), msgs.data(), msg_off.data(), idx.data(), m, sigs.data(), agg_off.data(), n,
                                                                      flags, seed, status.data()));
    else
      check_rc("bn254_batch_aggregate_verify_distinct_keyed",
               bn254_batch_aggregate_verify_distinct_keyed(e.raw(), msgs.data(), msg_off.data(), idx.data(), m, sigs.data(), agg_off.data(), n, 0,
                                                           status.data()));
    return status;
  }
  // opt-in randomised mode (include/bn254_hip.h: bn254_batch_verify_randomized): same result shape; non-zero entries
  // are exact, a zero is wrong with probability <= 2^-128 per group of 64 for a fresh secret 32-byte seed
  static std::vector<uint8_t> batch_verify_randomized(const std::vector<std::vector<uint8_t>>& messages, const std::vector<Signature>& signatures,
                                                      const std::vector<PublicKey>& public_keys, const std::array<uint8_t, 32>& seed,
                                                      Engine& e = Engine::default_engine()) {
    size_t n = messages.size();
    if (signatures.size() != n || public_keys.size() != n) throw Error(ErrorKind::InvalidLength);
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<uint8_t> msgs, sigs(n * 64), pks(n * 128), status(n, 0);
    for (size_t i = 0; i < n; ++i) {
      off[i] = msgs.size();
      msgs.insert(msgs.end(), messages[i].begin(), messages[i].end());
      std::memcpy(&sigs[64 * i], signatures[i].raw.data(), 64);
      std::memcpy(&pks[128 * i], public_keys[i].raw.data(), 128);
    }
    off[n] = msgs.size();
    check_rc("bn254_batch_verify_randomized",
             bn254_batch_verify_randomized(e.raw(), msgs.data(), off.data(), sigs.data(), pks.data(), n, 0, seed.data(), status.data(), nullptr));
    return status;
  }
};

inline void check_public_keys(const PublicKey& pk_g2, const PublicKeyG1& pk_g1, Engine& e = Engine::default_engine()) {
  uint8_t st = 0;
  check_rc("bn254_batch_check_public_keys", bn254_batch_check_public_keys(e.raw(), pk_g2.raw.data(), pk_g1.raw.data(), 1, 0, &st));
  check_status(st);
}

// The reference's precompile formatters (src/utils.rs:197-239): the two (G1, G2) pairs of the verification equation
// e(H(m), pk) * e(sig, -G2::one()) with every 32-byte big-endian coordinate byte-reversed (zeropool-bn's little-endian affine form), for an
// on-chain alt_bn128 pairing precompile.
struct PairingCheckValues {
  std::array<uint8_t, 64> g1[2];      // H(m), the signature
  std::array<uint8_t, 128> g2[2];     // the public key, -G2::one()
  bool operator==(const PairingCheckValues& o) const { return g1[0] == o.g1[0] && g1[1] == o.g1[1] && g2[0] == o.g2[0] && g2[1] == o.g2[1]; }
};
template <size_t N> inline std::array<uint8_t, N> le_chunks(const std::array<uint8_t, N>& be) {
  std::array<uint8_t, N> r{};
  for (size_t i = 0; i < N; i += 32) std::reverse_copy(be.begin() + i, be.begin() + i + 32, r.begin() + i);
  return r;
}
inline const PublicKey& neg_g2_one(Engine& e = Engine::default_engine()) {      // (r - 1) * G2::one()
  static const PublicKey neg = [&e] {
    PrivateKey k;
    const uint8_t r_minus_1[32] = {0x30, 0x64, 0x4E, 0x72, 0xE1, 0x31, 0xA0, 0x29, 0xB8, 0x50, 0x45, 0xB6, 0x81, 0x81, 0x58, 0x5D,
                                   0x28, 0x33, 0xE8, 0x48, 0x79, 0xB9, 0x70, 0x91, 0x43, 0xE1, 0xF5, 0x93, 0xF0, 0x00, 0x00, 0x00};
    std::memcpy(k.bytes.data(), r_minus_1, 32);
    return PublicKey::from_private_key(k, e);
  }();
  return neg;
}
inline PairingCheckValues pairing_check_values_of(const Signature& hash, const Signature& signature, const PublicKey& key, Engine& e) {
  PairingCheckValues v;
  v.g1[0] = le_chunks(hash.raw); v.g2[0] = le_chunks(key.raw);
  v.g1[1] = le_chunks(signature.raw); v.g2[1] = le_chunks(neg_g2_one(e).raw);
  return v;
}
// src/utils.rs:216-239: like the reference this does NOT validate the signature or the key (it only re-orders bytes); a message that does not
// hash throws its Error
inline PairingCheckValues format_pairing_check_uncompressed_values(const std::vector<uint8_t>& message, const Signature& signature, const PublicKey& public_key,
                                                                   Engine& e = Engine::default_engine()) {
  Signature h;
  const uint64_t off[2] = {0, message.size()};
  uint8_t st = 0;
  check_rc("bn254_batch_hash_to_g1", bn254_batch_hash_to_g1(e.raw(), message.data(), off, 1, h.raw.data(), &st, nullptr));
  check_status(st);
  return pairing_check_values_of(h, signature, public_key, e);
}
// src/utils.rs:197-214: the same from the COMPRESSED signature (33 B) and public key (65 B); both are decoded, and thereby validated, first
inline PairingCheckValues format_pairing_check_values(const std::vector<uint8_t>& message, const std::vector<uint8_t>& signature33,
                                                      const std::vector<uint8_t>& public_key65, Engine& e = Engine::default_engine()) {
  const Signature sig = Signature::from_compressed(signature33.data(), signature33.size(), e);
  const PublicKey pk = PublicKey::from_compressed(public_key65.data(), public_key65.size(), e);
  return format_pairing_check_uncompressed_values(message, sig, pk, e);
}
// format_pairing_check_uncompressed_values(message, signature, apk) for apk = the sum of the registered keys signer_indices names, from ONE
// device call (ECDSA::verify_keyed_signers_export).  Throws the item's Error for any non-zero status, VerificationFailed included — a failing
// aggregate is never formatted — and Error{PointInJacobian} for an identity aggregate key, as PublicKey::to_uncompressed does.
inline PairingCheckValues format_pairing_check_keyed_signers(const std::vector<uint8_t>& message, const Signature& signature,
                                                             const std::vector<uint32_t>& signer_indices, size_t n_keys,
                                                             Engine& e = Engine::default_engine()) {
  const ECDSA::ExportResult r = ECDSA::verify_keyed_signers_export(message, signature, signer_indices, n_keys, e);
  check_status(r.status);
  r.key.to_uncompressed();
  return pairing_check_values_of(r.hash, signature, r.key, e);
}
inline PairingCheckValues format_pairing_check_keyed_signers(const std::vector<uint8_t>& message, const CompressedSignature& signature,
                                                             const std::vector<uint32_t>& signer_indices, size_t n_keys,
                                                             Engine& e = Engine::default_engine()) {
  const ECDSA::ExportResult r = ECDSA::verify_keyed_signers_export(message, signature, signer_indices, n_keys, e);
  check_status(r.status);
  r.key.to_uncompressed();
  return pairing_check_values_of(r.hash, Signature::from_compressed(signature.raw.data(), signature.raw.size(), e), r.key, e);
}

}  // namespace bn254
