// A reshare through the C++ host API: a 3-of-5 committee hands its group key on to a 4-of-7 committee.  Old member i deals its share s_i
// with a polynomial g_i of degree 3, g_i(0) = s_i, and publishes the four commitments D_i = g_i's coefficients times G2; D_i,0 is its
// registered key.  The library qualifies the dealers, takes the three lowest, and combines their vectors under the Lagrange coefficients:
// C'_k = sum lambda_i D_i,k.  C'_0 is the old group key; the new committee is registered from the C'_k and passes the dealing check with
// that same key.  A dealer whose first commitment is not its key is left out, and the key still stays.
// (The dealings are done here in 128-bit integers — small coefficients, no reduction needed.  Producing them is not the library's job.)
// Needs an MI355X.
//   g++ -std=c++17 reshare_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o reshare_example
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
// the group order r, big-endian, minus a small value: the scalar -v
static std::array<uint8_t, 32> minus(uint8_t v) {
  std::array<uint8_t, 32> r = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                               0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xf0, 0x00, 0x00, 0x01};
  int borrow = v;
  for (int i = 31; i >= 0 && borrow; --i) {
    const int d = (int)r[i] - borrow;
    r[i] = (uint8_t)(d & 0xFF);
    borrow = d < 0 ? 1 : 0;
  }
  return r;
}
static std::array<uint8_t, 32> plus(uint8_t v) {
  std::array<uint8_t, 32> k{};
  k[31] = v;
  return k;
}
int main() {
  try {
    // the old committee: f of degree 2, five shares, the share keys registered from f's commitments
    const unsigned __int128 f[3] = {0x6b2f1c9d0f3a7e55ull, 0x1f83d9ab3c6ef372ull, 0x510e527fade682d1ull};
    const std::vector<bn254::PublicKey> old_commitments = commit(f, 3);
    if (bn254::ECDSA::register_keys_from_commitments(old_commitments, 5) != std::vector<uint8_t>(5, 0)) { printf("ERROR: old registration\n"); return 2; }
    // every old member's sub-dealing to the new committee: g_i(0) = its share
    std::vector<std::pair<uint32_t, std::vector<bn254::PublicKey>>> dealers;
    for (unsigned i = 0; i < 5; ++i) {
      const unsigned __int128 g[4] = {value_at(f, 3, i + 1), 0x9b05688c2b3e6c1full + 77 * i, 0x243f6a8885a308d3ull + 1001 * i, 0x13198a2e03707344ull + 5 * i};
      dealers.push_back({i, commit(g, 4)});
    }
    const bn254::ECDSA::Reshare all = bn254::ECDSA::reshare_commitments(dealers, 3, 5);
    if (all.used != std::vector<uint32_t>{0, 1, 2} || all.statuses != std::vector<uint8_t>(5, 0)) { printf("ERROR: selection\n"); return 3; }
    if (all.commitments.size() != 4 || all.commitments[0].raw != old_commitments[0].raw) { printf("ERROR: the group key moved\n"); return 4; }
    // the same by hand: the points 1, 2, 3 have the coefficients 3, -3, 1
    const std::vector<bn254::PublicKey> by_hand =
        bn254::ECDSA::g2_vector_combine({dealers[0].second, dealers[1].second, dealers[2].second}, {plus(3), minus(3), plus(1)});
    for (int k = 0; k < 4; ++k)
      if (by_hand[k].raw != all.commitments[k].raw) { printf("ERROR: commitment %d\n", k); return 5; }
    // dealer 0 publishes another member's key as D_0: left out, the next three are taken, the key stays
    std::vector<std::pair<uint32_t, std::vector<bn254::PublicKey>>> cheat = dealers;
    cheat[0].second[0] = dealers[1].second[0];
    const bn254::ECDSA::Reshare moved = bn254::ECDSA::reshare_commitments(cheat, 3, 5);
    if (moved.used != std::vector<uint32_t>{1, 2, 3} || moved.statuses[0] != (uint8_t)bn254::ErrorKind::VerificationFailed) { printf("ERROR: disqualification\n"); return 6; }
    if (moved.commitments[0].raw != old_commitments[0].raw) { printf("ERROR: the group key moved with S\n"); return 7; }
    // too few dealers
    try {
      bn254::ECDSA::reshare_commitments({dealers[0], dealers[4]}, 3, 5);
      printf("ERROR: two dealers passed\n");
      return 8;
    } catch (const bn254::ReshareFailed& e) {
      if (e.qualified != std::vector<uint32_t>{0, 4}) { printf("ERROR: qualified set\n"); return 9; }
    }
    // the new committee: seven share keys from the four commitments, the group key named, the dealing check passes with it
    if (bn254::ECDSA::register_keys_from_commitments(all.commitments, 7, /*register_key=*/true) != std::vector<uint8_t>(7, 0)) { printf("ERROR: new registration\n"); return 10; }
    std::array<uint8_t, 32> seed{};
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(31 * i + 7);
    if (bn254::ECDSA::check_dealing(4, seed).raw != old_commitments[0].raw) { printf("ERROR: new dealing\n"); return 11; }
    printf("reshare: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
