// Feldman commitments through the C++ host API: a dealer shares a secret 3-of-5 and publishes, beside the five shares, the commitments
// C_k = a_k * G2 of its polynomial f(X) = a_0 + a_1 X + a_2 X^2.  Every holder checks the share it received against the commitments
// (share * G2 == the vector at index + 1); the committee derives the five share keys from the three commitments on the device and
// registers them in one call, names C_0 as the group key, and the key set then passes the dealing check by construction.  Two dealers'
// vectors add up to the commitments of the summed polynomial (a DKG's last step).
// (The dealing is done here in 128-bit integers — small coefficients, no reduction needed.  Producing a dealing is not the library's job.)
// Needs an MI355X.
//   g++ -std=c++17 commitments_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o commitments_example
#include <cstdio>
#include "bn254.hpp"

static bn254::PrivateKey key_of(unsigned __int128 v) {
  bn254::PrivateKey k;
  for (int i = 0; i < 16; ++i) k.bytes[31 - i] = (uint8_t)(v >> (8 * i));
  return k;
}
static unsigned __int128 value_at(const unsigned __int128* a, int t, unsigned x) {
  unsigned __int128 f = 0, xe = 1;
  for (int e = 0; e < t; ++e) { f += a[e] * xe; xe *= x; }
  return f;
}
static std::vector<bn254::PublicKey> commit(const unsigned __int128* a, int t) {
  std::vector<bn254::PublicKey> c;
  for (int k = 0; k < t; ++k) c.push_back(bn254::PublicKey::from_private_key(key_of(a[k])));
  return c;
}
int main() {
  try {
    const unsigned __int128 a[3] = {0x6b2f1c9d0f3a7e55ull, 0x1f83d9ab3c6ef372ull, 0x510e527fade682d1ull};
    const unsigned __int128 b[3] = {0x9b05688c2b3e6c1full, 0x243f6a8885a308d3ull, 0x13198a2e03707344ull};
    const std::vector<bn254::PublicKey> ca = commit(a, 3), cb = commit(b, 3);
    // the values at 0 and at 1 .. 5: C_0 itself and the five share keys
    const std::vector<bn254::PublicKey> values = bn254::ECDSA::commitments_eval(ca, {0, 1, 2, 3, 4, 5});
    if (values[0].raw != ca[0].raw) { printf("ERROR: x = 0\n"); return 2; }
    for (unsigned j = 0; j < 5; ++j)
      if (values[j + 1].raw != bn254::PublicKey::from_private_key(key_of(value_at(a, 3, j + 1))).raw) { printf("ERROR: share key %u\n", j); return 3; }
    // holder 3 checks what the two dealers sent it; dealer b's share is off by one
    const std::vector<uint8_t> verdicts =
        bn254::ECDSA::batch_verify_dealt_shares({ca, cb}, 3, {key_of(value_at(a, 3, 4)), key_of(value_at(b, 3, 4) + 1)});
    if (verdicts != std::vector<uint8_t>{0, (uint8_t)bn254::ErrorKind::VerificationFailed}) { printf("ERROR: share check\n"); return 4; }
    // the committee registers the share keys straight from the commitments and names C_0
    if (bn254::ECDSA::register_keys_from_commitments(ca, 5, /*register_key=*/true) != std::vector<uint8_t>(5, 0)) { printf("ERROR: registration\n"); return 5; }
    std::array<uint8_t, 32> seed{};
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(29 * i + 5);
    if (bn254::ECDSA::check_dealing(3, seed).raw != ca[0].raw) { printf("ERROR: dealing check\n"); return 6; }
    // both dealers qualified: the commitments of a + b
    unsigned __int128 sum[3];
    for (int k = 0; k < 3; ++k) sum[k] = a[k] + b[k];
    const std::vector<bn254::PublicKey> both = bn254::ECDSA::combine_commitments({ca, cb}), want = commit(sum, 3);
    for (int k = 0; k < 3; ++k)
      if (both[k].raw != want[k].raw) { printf("ERROR: combined commitment %d\n", k); return 7; }
    if (bn254::ECDSA::register_keys_from_commitments(both, 5) != std::vector<uint8_t>(5, 0) || bn254::ECDSA::check_dealing(3, seed).raw != want[0].raw) {
      printf("ERROR: combined dealing\n");
      return 8;
    }
    // a commitment off the curve: its decode error, and no keys left registered
    std::vector<bn254::PublicKey> bad = ca;
    bad[1].raw[100] ^= 4;
    try {
      bn254::ECDSA::register_keys_from_commitments(bad, 5);
      printf("ERROR: a bad commitment passed\n");
      return 9;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::InvalidGroupPoint) { printf("ERROR: wrong error\n"); return 10; }
    }
    printf("commitments: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
