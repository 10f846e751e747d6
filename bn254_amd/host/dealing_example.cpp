// Checking a dealing through the C++ host API: a committee of five receives share keys from a dealer who says they are a 3-of-5 dealing —
// key j = f(j + 1) * G2 for one polynomial f of degree 2.  Before it signs anything the committee registers the keys and asks the library:
// do they lie on one polynomial of degree below 3, and which group key do they interpolate to?  An honest dealing passes under every seed and
// gives f(0) * G2; one key off the polynomial, or a polynomial of degree 3, is refused with VerificationFailed.  The seed must be drawn
// AFTER the keys are fixed (here a constant, for the example's sake).
// (The dealing is done here in 128-bit integers — small coefficients, no reduction needed.  Producing a dealing is not the library's job.)
// Needs an MI355X.
//   g++ -std=c++17 dealing_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o dealing_example
#include <cstdio>
#include "bn254.hpp"

static bn254::PrivateKey key_of(unsigned __int128 v) {
  bn254::PrivateKey k;
  for (int i = 0; i < 16; ++i) k.bytes[31 - i] = (uint8_t)(v >> (8 * i));
  return k;
}
static std::vector<bn254::PublicKey> deal(const unsigned __int128* a, int degree, unsigned n) {
  std::vector<bn254::PublicKey> pks;
  for (unsigned j = 0; j < n; ++j) {
    unsigned __int128 x = j + 1, f = 0, xe = 1;
    for (int e = 0; e <= degree; ++e) { f += a[e] * xe; xe *= x; }
    pks.push_back(bn254::PublicKey::from_private_key(key_of(f)));
  }
  return pks;
}
static bool refused(uint32_t threshold, const std::array<uint8_t, 32>& seed) {
  try {
    bn254::ECDSA::check_dealing(threshold, seed);
    return false;
  } catch (const bn254::Error& e) { return e.kind == bn254::ErrorKind::VerificationFailed; }
}
int main() {
  try {
    const unsigned __int128 a[4] = {0x6b2f1c9d0f3a7e55ull, 0x1f83d9ab3c6ef372ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full};
    std::array<uint8_t, 32> seed{};
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(17 * i + 3);
    const bn254::PublicKey group_key = bn254::PublicKey::from_private_key(key_of(a[0]));
    std::vector<bn254::PublicKey> pks = deal(a, 2, 5);
    if (bn254::ECDSA::register_keys(pks) != std::vector<uint8_t>(5, 0)) { printf("ERROR: registration\n"); return 2; }
    uint32_t bad = 0;
    const bn254::PublicKey k = bn254::ECDSA::check_dealing(3, seed, /*register_key=*/true, &bad);
    if (k.raw != group_key.raw || bad != UINT32_MAX) { printf("ERROR: group key\n"); return 3; }
    seed[0] ^= 1;
    if (bn254::ECDSA::check_dealing(3, seed).raw != group_key.raw) { printf("ERROR: another seed\n"); return 4; }
    // the same keys are a 4-of-5 dealing too (degree 2 is below 4), with the same group key; they are no 2-of-5 dealing
    if (bn254::ECDSA::check_dealing(4, seed).raw != group_key.raw || !refused(2, seed)) { printf("ERROR: other thresholds\n"); return 5; }
    // the group key is the weighted sum of the first three keys under the coefficients 3, -3, 1 of the points 1, 2, 3
    std::vector<std::array<uint8_t, 32>> lam(3);
    for (auto& l : lam) l.fill(0);
    lam[0][31] = 3; lam[2][31] = 1;
    static const uint8_t minus3[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                                       0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xef, 0xff, 0xff, 0xfe};   // r - 3
    std::memcpy(lam[1].data(), minus3, 32);
    if (bn254::ECDSA::g2_msm({pks[0], pks[1], pks[2]}, lam).raw != group_key.raw) { printf("ERROR: g2_msm\n"); return 6; }
    // one key off the polynomial: refused; a dealing of degree 3: refused as 3-of-5
    std::vector<bn254::PublicKey> off = pks;
    off[4] = bn254::PublicKey::from_private_key(key_of(12345));
    if (bn254::ECDSA::register_keys(off) != std::vector<uint8_t>(5, 0) || !refused(3, seed)) { printf("ERROR: a replaced key passed\n"); return 7; }
    if (bn254::ECDSA::register_keys(deal(a, 3, 5)) != std::vector<uint8_t>(5, 0) || !refused(3, seed)) { printf("ERROR: degree 3 passed\n"); return 8; }
    printf("dealing check: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
