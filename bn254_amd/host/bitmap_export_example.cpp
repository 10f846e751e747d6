// A relayer's hop through the C++ host API: four validators with voting weights sign a message, the aggregate arrives with the bitmap of its
// signers, and the relayer needs what a verifier WITHOUT the validator set takes — the aggregate public key, H(m), the precompile input —
// and the weight behind the bitmap to compare with its quorum.  One export call returns them with the verdict.
// Needs an MI355X.
//   g++ -std=c++17 bitmap_export_example.cpp -L.. -lbn254hip -Wl,-rpath,'$ORIGIN/..' -o bitmap_export_example
#include <cstdio>
#include "bn254.hpp"

int main() {
  try {
    bn254::PrivateKey k[4];
    std::vector<bn254::PublicKey> pk;
    for (int j = 0; j < 4; ++j) {
      k[j].bytes = {};
      k[j].bytes[31] = (uint8_t)(21 + j);
      k[j].bytes[9] = 0x3c;
      pk.push_back(bn254::PublicKey::from_private_key(k[j]));
    }
    if (bn254::ECDSA::register_keys(pk) != std::vector<uint8_t>{0, 0, 0, 0}) { printf("ERROR: registration\n"); return 2; }
    bn254::ECDSA::register_key_weights({10, 20, 30, 40});
    const std::vector<uint8_t> m = {'e', 'p', 'o', 'c', 'h', ' ', '7'};
    const std::vector<uint32_t> signers = {0, 2, 3};
    const bn254::Signature sigma = bn254::ECDSA::sign(m, k[0]) + bn254::ECDSA::sign(m, k[2]) + bn254::ECDSA::sign(m, k[3]);
    // the aggregate key alone, and the same key from host-side additions
    const bn254::PublicKey apk = bn254::ECDSA::aggregate_public_key_signers(signers, 4);
    if (!(apk == pk[0] + pk[2] + pk[3])) { printf("ERROR: aggregate key\n"); return 3; }
    if (bn254::ECDSA::batch_aggregate_public_keys_signers({{1, 7}}, 4)[0].status != 2) { printf("ERROR: index outside the set\n"); return 4; }
    // the quorum: 10 + 30 + 40 of 100
    if (bn254::ECDSA::signers_weight(signers, 4) != 80) { printf("ERROR: weight\n"); return 5; }
    // the verify that returns what it computed
    const auto r = bn254::ECDSA::verify_keyed_signers_export(m, sigma, signers, 4);
    if (r.status != 0 || !(r.key == apk) || r.hash.is_identity()) { printf("ERROR: export\n"); return 6; }
    const auto bad = bn254::ECDSA::verify_keyed_signers_export(m, sigma, {0, 2}, 4);
    if (bad.status != 9 || !(bad.key == pk[0] + pk[2]) || bad.hash.raw != r.hash.raw) { printf("ERROR: export of a failing aggregate\n"); return 7; }
    // the precompile input from that one call equals the formatter on (m, sigma, apk); compressed sigma gives the same
    const bn254::PairingCheckValues v = bn254::format_pairing_check_keyed_signers(m, sigma, signers, 4);
    if (!(v == bn254::format_pairing_check_uncompressed_values(m, sigma, apk))) { printf("ERROR: formatter\n"); return 8; }
    if (v.g1[0] != bn254::le_chunks(r.hash.raw) || v.g2[0] != bn254::le_chunks(apk.raw)) { printf("ERROR: layout\n"); return 9; }
    const std::array<uint8_t, 33> c = sigma.to_compressed();
    if (!(v == bn254::format_pairing_check_keyed_signers(m, bn254::CompressedSignature::from_bytes(c.data(), c.size()), signers, 4))) { printf("ERROR: compressed\n"); return 10; }
    try {
      bn254::format_pairing_check_keyed_signers(m, sigma, {0, 2}, 4);
      printf("ERROR: a failing aggregate was formatted\n");
      return 11;
    } catch (const bn254::Error& e) {
      if (e.kind != bn254::ErrorKind::VerificationFailed) return 12;
    }
    // a registration forgets the weights
    bn254::ECDSA::register_keys(pk);
    try {
      bn254::ECDSA::signers_weight(signers, 4);
      printf("ERROR: weights survived a registration\n");
      return 13;
    } catch (const bn254::NativeError&) {}
    printf("bitmap export: ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
