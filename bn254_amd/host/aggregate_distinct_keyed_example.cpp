// Aggregates over distinct messages against REGISTERED keys through the C++ host API: three validators are registered once, each signs its
// own message, and the sum verifies against (message, key index) pairs; swapped indices and an index outside the set are rejected.
// Needs an MI355X.
//   g++ -std=c++17 aggregate_distinct_keyed_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o aggregate_distinct_keyed_example
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
    for (auto& sk : k) pks.push_back(bn254::PublicKey::from_private_key(sk));
    if (bn254::ECDSA::register_keys(pks) != std::vector<uint8_t>{0, 0, 0}) { printf("ERROR: registration\n"); return 5; }
    std::vector<uint8_t> m0 = {'v', ' ', '0'}, m1 = {'v', ' ', '1'}, m2 = {'v', ' ', '2'};
    auto sigma = bn254::ECDSA::sign(m0, k[0]) + bn254::ECDSA::sign(m1, k[1]) + bn254::ECDSA::sign(m2, k[2]);
    bn254::ECDSA::aggregate_verify_keyed({m0, m1, m2}, sigma, {0, 1, 2});
    try {
      bn254::ECDSA::aggregate_verify_keyed({m0, m1, m2}, sigma, {1, 0, 2});
      printf("ERROR: swapped indices accepted\n");
      return 2;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::VerificationFailed) return 3;
    }
    auto st = bn254::ECDSA::batch_aggregate_verify_distinct_keyed({{{m0, m1, m2}, sigma, {0, 1, 2}}, {{m0}, sigma, {0}}, {{m0, m1}, sigma, {0, 3}},
                                                                   {{}, bn254::Signature{}, {}}});
    if (st != std::vector<uint8_t>{0, 9, 2, 0}) { printf("ERROR: batch statuses\n"); return 4; }
    printf("keyed aggregate over distinct messages: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
