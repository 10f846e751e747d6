// Compressed G1 input of the registered-key calls (include/bn254_hip.h: BN254_FLAG_G1_COMPRESSED) and bn254_batch_g1_decompress_device: the
// per-item bodies of the kernels of bn254_g1stage.hip, shared with their host compilation for the CPU suite (tests/hostsim, plain, under
// sanitizers and under -DBN_TRACK_BOUNDS).  Include after bn254_io.h.
//   * STAGE: encoding c -> 64 bytes S(c) and one pre-status byte.  (st, u) = decompress_g1(c), in from_compressed's order (x >= q: 6, no
//     square root: 6, only then a bad prefix: 3).  st == 0: S(c) = u, pre = 0.  Else S(c) = BE32(q) || 32 zero bytes, pre = st: the x of the
//     stand-in is out of range, so every uncompressed decoder reads 6 there under every flags value (decode_g1: not all zero, a coordinate
//     >= q), and no route verifies, takes, counts or queues the item.
//   * OVERLAY, behind the call: status = pre where pre != 0 and the call wrote 6.  That 6 can only be the stand-in's own decode status (the
//     one rule that comes before an item's decode, the fill with 2 of an item of no accepted tuple, keeps its 2).
// The byte loads of the encodings are unaligned (33-byte stride); the 64-byte outputs are written as words and must be 4-byte aligned.
#pragma once

namespace bn254 {

// the stand-in of an encoding that does not decompress
BN_DEV void g1c_stand_in(uint8_t* out64) {
  uint32_t* w = (uint32_t*)out64;
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = __builtin_bswap32(C_Q[7 - i]);
#pragma unroll
  for (int i = 8; i < 16; ++i) w[i] = 0;
}
// item of the staging kernel: out64 = S(c); returns the pre-status
BN_DEV uint8_t g1c_stage_item(uint8_t* out64, const uint8_t* in33) {
  G1Affine p;
  const uint8_t st = decompress_g1(p, in33);
  if (st == ST_OK) encode_g1(out64, p);
  else g1c_stand_in(out64);
  return st;
}
// item of the overlay kernel
BN_DEV uint8_t g1c_overlay_item(uint8_t status, uint8_t pre) { return pre != ST_OK && status == ST_NOT_MEMBER ? pre : status; }
// item of bn254_batch_g1_decompress_device: the bytes of the host form (a failed item: 64 zero bytes); returns the status
BN_DEV uint8_t g1c_decompress_item(uint8_t* out64, const uint8_t* in33) {
  G1Affine p;
  const uint8_t st = decompress_g1(p, in33);
  if (st != ST_OK) p.inf = true;
  encode_g1(out64, p);
  return st;
}

}  // namespace bn254
