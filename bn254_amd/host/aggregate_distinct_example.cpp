// Aggregate signatures over DISTINCT messages through the C++ host API: two signers sign different messages, the sum of their signatures
// verifies against both (message, key) pairs, and the same aggregate with the pairs swapped is rejected.  Needs an MI355X.
//   g++ -std=c++17 aggregate_distinct_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o aggregate_distinct_example
#include <cstdio>
#include "bn254.hpp"

static std::array<uint8_t, 32> unhex(const char* s) {
  std::array<uint8_t, 32> o{};
  for (int i = 0; i < 32; ++i) { unsigned v; sscanf(s + 2 * i, "%2x", &v); o[i] = (uint8_t)v; }
  return o;
}
int main() {
  try {
    bn254::PrivateKey k1, k2;
    k1.bytes = unhex("c9afa9d845ba75166b5c215767b1d6934e50c3db36e89b127b8a622b120f6721");
    k2.bytes = unhex("a55e93edb1350916bf5beea1b13d8f198ef410033445bcb645b65be5432722f1");
    auto pk1 = bn254::PublicKey::from_private_key(k1), pk2 = bn254::PublicKey::from_private_key(k2);
    std::vector<uint8_t> m1 = {'t', 'x', ' ', '1'}, m2 = {'t', 'x', ' ', '2'};
    auto sigma = bn254::ECDSA::sign(m1, k1) + bn254::ECDSA::sign(m2, k2);
    bn254::ECDSA::aggregate_verify({m1, m2}, sigma, {pk1, pk2});
    try {
      bn254::ECDSA::aggregate_verify({m2, m1}, sigma, {pk1, pk2});
      printf("ERROR: swapped pairs accepted\n");
      return 2;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::VerificationFailed) return 3;
    }
    auto st = bn254::ECDSA::batch_aggregate_verify_distinct({{{m1, m2}, sigma, {pk1, pk2}}, {{m1}, sigma, {pk1}}, {{}, bn254::Signature{}, {}}});
    if (st != std::vector<uint8_t>{0, 9, 0}) { printf("ERROR: batch statuses\n"); return 4; }
    printf("aggregate over distinct messages: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
