// Proofs of possession through the C++ host API: three validators prove their keys, the set is registered with its proofs, and an aggregate
// of all three verifies; then the second validator presents the first one's proof: its key is refused with VerificationFailed at
// registration, an aggregate that names it is refused, and the other two still verify.
// Needs an MI355X.
//   g++ -std=c++17 pop_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o pop_example
#include <cstdio>
#include "bn254.hpp"

static std::array<uint8_t, 32> unhex(const char* s) {
  std::array<uint8_t, 32> o{};
  for (int i = 0; i < 32; ++i) { unsigned v; sscanf(s + 2 * i, "%2x", &v); o[i] = (uint8_t)v; }
  return o;
}
int main() {
  try {
    bn254::PrivateKey k[3];
    k[0].bytes = unhex("c9afa9d845ba75166b5c215767b1d6934e50c3db36e89b127b8a622b120f6721");
    k[1].bytes = unhex("a55e93edb1350916bf5beea1b13d8f198ef410033445bcb645b65be5432722f1");
    k[2].bytes = unhex("1f7c2d8b5e9a3c4d6e0f1a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f");
    std::vector<bn254::PublicKey> pks;
    std::vector<bn254::Signature> pops;
    for (auto& sk : k) { pks.push_back(bn254::PublicKey::from_private_key(sk)); pops.push_back(bn254::ECDSA::prove_possession(sk)); }
    bn254::ECDSA::verify_possession(pks[0], pops[0]);
    try {
      bn254::ECDSA::verify_possession(pks[1], pops[0]);
      printf("ERROR: another key's proof accepted\n");
      return 2;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::VerificationFailed) return 3;
    }
    if (bn254::ECDSA::register_keys_proven(pks, pops) != std::vector<uint8_t>{0, 0, 0}) { printf("ERROR: proven registration\n"); return 4; }
    std::vector<uint8_t> m = {'b', 'l', 'o', 'c', 'k', ' ', '7'};
    auto sigma = bn254::ECDSA::sign(m, k[0]) + bn254::ECDSA::sign(m, k[1]) + bn254::ECDSA::sign(m, k[2]);
    bn254::ECDSA::verify_keyed_signers(m, sigma, {0, 1, 2}, 3);
    // the second validator without a proof of its own
    if (bn254::ECDSA::register_keys_proven(pks, {pops[0], pops[0], pops[2]}) != std::vector<uint8_t>{0, 9, 0}) { printf("ERROR: unproven key registered\n"); return 5; }
    try {
      bn254::ECDSA::verify_keyed_signers(m, sigma, {0, 1, 2}, 3);
      printf("ERROR: aggregate over an unproven key accepted\n");
      return 6;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::VerificationFailed) return 7;
    }
    bn254::ECDSA::verify_keyed_signers(m, bn254::ECDSA::sign(m, k[0]) + bn254::ECDSA::sign(m, k[2]), {0, 2}, 3);
    printf("proofs of possession: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
