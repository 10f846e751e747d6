// Signatures as they arrive off the wire — 33 bytes, 0x02 / 0x03 || x — through the registered-key calls of the C++ host API, never decoded on
// the host: four validators sign a message, an aggregator collects the compressed shares into one signer-bitmap aggregate (one share arrives
// with a damaged prefix byte and one is not a point at all: each reads the status Signature::from_compressed would have thrown and is left
// out), and the aggregate, compressed again for the next hop, verifies against the keys that signed.
// Needs an MI355X.
//   g++ -std=c++17 compressed_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o compressed_example
#include <cstdio>
#include "bn254.hpp"

int main() {
  try {
    bn254::PrivateKey k[4];
    std::vector<bn254::PublicKey> pk;
    for (int j = 0; j < 4; ++j) {
      k[j].bytes = {};
      k[j].bytes[31] = (uint8_t)(11 + j);
      k[j].bytes[7] = 0x5a;
      pk.push_back(bn254::PublicKey::from_private_key(k[j]));
    }
    if (bn254::ECDSA::register_keys(pk) != std::vector<uint8_t>{0, 0, 0, 0}) { printf("ERROR: registration\n"); return 2; }
    const std::vector<uint8_t> m = {'b', 'l', 'o', 'c', 'k', ' ', '1', '2'};
    std::vector<bn254::CompressedSignature> wire;
    for (int j = 0; j < 4; ++j) {
      const std::array<uint8_t, 33> c = bn254::ECDSA::sign(m, k[j]).to_compressed();
      wire.push_back(bn254::CompressedSignature::from_bytes(c.data(), c.size()));
    }
    try {
      bn254::CompressedSignature::from_bytes(wire[0].raw.data(), 32);
      printf("ERROR: 32 bytes accepted\n");
      return 3;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::InvalidEncoding) return 4;
    }
    wire[1].raw[0] = 0x04;                                     // a prefix that is neither 0x02 nor 0x03: InvalidEncoding (3)
    for (int i = 1; i < 33; ++i) wire[3].raw[i] = 0xff;        // x >= q: NotMemberError (6)
    // collect: the statuses of the four shares, the aggregate of the two that are valid, and who signed
    auto r = bn254::ECDSA::aggregate_keyed_signers(m, wire, {0, 1, 2, 3}, 4);
    if (r.statuses != std::vector<uint8_t>{0, 3, 0, 6} || r.signer_indices != std::vector<uint32_t>{0, 2}) { printf("ERROR: collect\n"); return 5; }
    // the same call on decoded signatures gives the same aggregate
    auto plain = bn254::ECDSA::aggregate_keyed_signers(m, {bn254::ECDSA::sign(m, k[0]), bn254::ECDSA::sign(m, k[2])}, {0, 2}, 4);
    if (plain.signature.raw != r.signature.raw) { printf("ERROR: aggregates differ\n"); return 6; }
    // the next hop: the aggregate travels compressed, and is verified against the bitmap of its signers as it is
    const std::array<uint8_t, 33> c = r.signature.to_compressed();
    const bn254::CompressedSignature sigma = bn254::CompressedSignature::from_bytes(c.data(), c.size());
    bn254::ECDSA::verify_keyed_signers(m, sigma, r.signer_indices, 4);
    try {
      bn254::ECDSA::verify_keyed_signers(m, sigma, {0, 1, 2}, 4);
      printf("ERROR: wrong signers accepted\n");
      return 7;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::VerificationFailed) return 8;
    }
    bn254::CompressedSignature flipped = sigma;
    flipped.raw[0] ^= 1;                                       // the other root: -sigma, a valid point that does not verify
    auto st = bn254::ECDSA::batch_verify_keyed_signers({{m, sigma, r.signer_indices}, {m, flipped, r.signer_indices}, {m, wire[1], {1}}}, 4);
    if (st != std::vector<uint8_t>{0, 9, 3}) { printf("ERROR: bitmap verify\n"); return 9; }
    printf("compressed shares: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
