// A 2-of-3 threshold signature through the C++ host API: a dealer shares the group secret by f(x) = a0 + a1 x, validator j holds f(j + 1)
// and registers f(j + 1) * G2; any two validators' shares of a message interpolate to THE signature under a0 * G2, whichever two they are;
// one share alone, or a share that does not verify among two, is refused with VerificationFailed.
// (The dealing is done here in 128-bit integers for the example's sake — small coefficients, no reduction needed.  A deployment deals with a
// DKG or a trusted dealer of its own; the library checks every share against its registered key, not that the keys lie on one polynomial.)
// Needs an MI355X.
//   g++ -std=c++17 threshold_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o threshold_example
#include <cstdio>
#include "bn254.hpp"

static bn254::PrivateKey key_of(unsigned __int128 v) {
  bn254::PrivateKey k;
  for (int i = 0; i < 16; ++i) k.bytes[31 - i] = (uint8_t)(v >> (8 * i));
  return k;
}
int main() {
  try {
    const unsigned __int128 a0 = 0x6b2f1c9d0f3a7e55ull, a1 = 0x1f83d9ab3c6ef372ull;
    const bn254::PublicKey group_key = bn254::PublicKey::from_private_key(key_of(a0));
    bn254::PrivateKey share_sk[3];
    std::vector<bn254::PublicKey> share_pk;
    for (unsigned j = 0; j < 3; ++j) {
      share_sk[j] = key_of(a0 + a1 * (j + 1));                          // key index j stands for the evaluation point j + 1
      share_pk.push_back(bn254::PublicKey::from_private_key(share_sk[j]));
    }
    if (bn254::ECDSA::register_keys(share_pk) != std::vector<uint8_t>{0, 0, 0}) { printf("ERROR: registration\n"); return 2; }
    std::vector<uint8_t> m = {'b', 'l', 'o', 'c', 'k', ' ', '9'};
    bn254::Signature s[3];
    for (int j = 0; j < 3; ++j) s[j] = bn254::ECDSA::sign(m, share_sk[j]);
    auto r02 = bn254::ECDSA::threshold_combine_keyed(m, {s[2], s[0]}, {2, 0}, 3, 2);
    bn254::ECDSA::verify(m, r02.signature, group_key);
    if (r02.signer_indices != std::vector<uint32_t>{0, 2}) { printf("ERROR: keys used\n"); return 3; }
    auto r12 = bn254::ECDSA::threshold_combine_keyed(m, {s[1], s[2]}, {1, 2}, 3, 2);
    auto all = bn254::ECDSA::threshold_combine_keyed(m, {s[0], s[1], s[2]}, {0, 1, 2}, 3, 2);      // the two lowest are used
    if (r12.signature.raw != r02.signature.raw || all.signature.raw != r02.signature.raw || all.signer_indices != std::vector<uint32_t>{0, 1}) {
      printf("ERROR: subsets disagree\n");
      return 4;
    }
    // validator 1 sends validator 0's share: it does not verify under key 1, and one valid share is not enough
    auto bad = bn254::ECDSA::batch_threshold_combine_keyed({{m, {s[0], s[0]}, {0, 1}}}, 3, 2)[0];
    if (bad.status != 9 || bad.statuses != std::vector<uint8_t>{0, 9} || bad.signer_indices != std::vector<uint32_t>{0}) { printf("ERROR: bad share\n"); return 5; }
    try {
      bn254::ECDSA::threshold_combine_keyed(m, {s[1]}, {1}, 3, 2);
      printf("ERROR: one share accepted\n");
      return 6;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::VerificationFailed) return 7;
    }
    printf("threshold signatures: ok\n");
    // the optimistic form: interpolate first, verify the result once under the group key.  (Option 46 = 0 sends even this tiny call down
    // the optimistic route; by default a call this small takes the exact one, with the same bytes.)
    bn254::Engine& eng = bn254::Engine::default_engine();
    eng.set_option(BN254_OPT_THRESHOLD_OPT_MIN_SHARES, 0);
    try {
      bn254::ECDSA::threshold_combine_keyed_optimistic(m, {s[2], s[0]}, {2, 0}, 3, 2);
      printf("ERROR: accepted without a group key\n");
      return 8;
    } catch (const std::runtime_error&) {}
    bn254::ECDSA::register_group_key(group_key);
    auto o02 = bn254::ECDSA::threshold_combine_keyed_optimistic(m, {s[2], s[0]}, {2, 0}, 3, 2);
    auto oall = bn254::ECDSA::threshold_combine_keyed_optimistic(m, {s[0], s[1], s[2]}, {0, 1, 2}, 3, 2);
    uint64_t did[4];
    if (bn254_debug_threshold_opt_last(eng.raw(), did) != 0 || did[0] != 1 || did[1] != 1 || did[2] != 0) { printf("ERROR: the route did not run\n"); return 9; }
    if (o02.signature.raw != r02.signature.raw || oall.signature.raw != r02.signature.raw || oall.signer_indices != std::vector<uint32_t>{0, 1}) {
      printf("ERROR: optimistic result\n");
      return 10;
    }
    // the bad share again: the result does not verify under the group key, so the item goes the exact way — the exact call's answer
    auto obad = bn254::ECDSA::batch_threshold_combine_keyed_optimistic({{m, {s[0], s[0]}, {0, 1}}}, 3, 2)[0];
    if (obad.status != 9 || obad.statuses != bad.statuses || obad.signer_indices != bad.signer_indices) { printf("ERROR: optimistic bad share\n"); return 11; }
    printf("optimistic: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
