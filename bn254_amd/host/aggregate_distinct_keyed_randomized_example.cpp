// Randomised verification of many aggregates over distinct messages against REGISTERED keys through the C++ host API: three validators
// are registered once, four aggregates are verified in one call whose group checks are combined under random weights; the statuses are
// those of the exact call (a wrong sum and an index outside the set are rejected).  Needs an MI355X.
//   g++ -std=c++17 aggregate_distinct_keyed_randomized_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o aggregate_distinct_keyed_randomized_example
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
    // a batch this small takes the exact route by default (BN254_OPT_AGG_RAND_MIN_PAIRS); force the randomised one to show it
    bn254::Engine& e = bn254::Engine::default_engine();
    if (bn254_ctx_set_option(e.raw(), BN254_OPT_AGG_RAND_MIN_PAIRS, 0) != 0) { printf("ERROR: option\n"); return 6; }
    std::vector<uint8_t> m0 = {'v', ' ', '0'}, m1 = {'v', ' ', '1'}, m2 = {'v', ' ', '2'};
    auto s0 = bn254::ECDSA::sign(m0, k[0]), s1 = bn254::ECDSA::sign(m1, k[1]), s2 = bn254::ECDSA::sign(m2, k[2]);
    const std::array<uint8_t, 32> seed = unhex("0f1e2d3c4b5a69788796a5b4c3d2e1f00112233445566778899aabbccddeeff0");   // use a fresh secret seed
    std::vector<bn254::ECDSA::KeyedAggregate> batch = {{{m0, m1, m2}, s0 + s1 + s2, {0, 1, 2}}, {{m1, m2}, s1 + s2, {1, 2}},
                                                        {{m0, m1}, s0 + s2, {0, 1}}, {{m0, m1}, s0 + s1, {0, 3}}};
    const std::vector<uint8_t> want = {0, 0, 9, 2};
    if (bn254::ECDSA::batch_aggregate_verify_distinct_keyed(batch) != want) { printf("ERROR: exact statuses\n"); return 4; }
    if (bn254::ECDSA::batch_aggregate_verify_distinct_keyed_randomized(batch, seed) != want) { printf("ERROR: randomised statuses\n"); return 3; }
    if (bn254::ECDSA::batch_aggregate_verify_distinct_keyed_randomized(batch, seed, e, true) != want) { printf("ERROR: 64-bit statuses\n"); return 2; }
    uint64_t last[6];
    if (bn254_debug_agg_rand_last(e.raw(), last) != 0 || last[0] != 1) { printf("ERROR: the randomised route did not run\n"); return 7; }
    printf("keyed aggregates over distinct messages, randomised: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
