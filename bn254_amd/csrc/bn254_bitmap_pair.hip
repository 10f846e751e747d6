// Translation unit of libbn254hip.so: the aggregate key of a signer bitmap on LANE PAIRS (include/bn254_hip.h:
// bn254_batch_verify_keyed_bitmap[_device]; host side and the one-lane form: bn254_bitmap.hip; the walk itself: bn254_bitmap.h).  Compiled
// with the Fq2 layout of bn254_pair.hip, as bn254_aggkeyed.hip is, in a code object of its own: the kernels of bn254_pair.hip keep their
// code and their placement.  Reference: the sum is `Add for PublicKey` (/root/reference/src/types.rs:126-132).
#include <hip/hip_runtime.h>

#define BN_SPLIT_FP2 1
#ifndef BN_PAIR_NO_SQR_DPP_ASM
#define BN_PAIR_SQR_DPP_ASM 1
#endif
#define bn254 bn254_bmp   // own namespace, as in bn254_fe.hip
#include "bn254_pairing.h"
#include "bn254_bitmap.h"

using namespace bn254;

#include "bn254_ws.h"

#ifndef BN_PAIR_WG
#define BN_PAIR_WG 256
#endif
#define KERNEL_PAIR __global__ __launch_bounds__(BN_PAIR_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))

// One tuple per lane pair: the pair walks the tuple's bitmap (both lanes read the same words), adds one table entry per non-zero byte —
// or, without tables, one key per set bit — into a G2 sum kept in LDS (27 words per lane: the additions take it by reference), and writes
// the sum into the Q planes of workspace index i, where the verify kernels read tuple i's public key, with the identity flag; rule 2's
// status goes behind the signature's decode status (decoded before this kernel runs) into BY_ST_DECODE.  No early return: the additions
// vote across the wave.
KERNEL_PAIR void k_bm_sum_pair(const uint32_t* bits, size_t bm_words, size_t n, BmKeys K, const int32_t* rec, const uint8_t* rec_inf, Ws ws) {
  const unsigned role = threadIdx.x & 1u;
  const size_t i = ((size_t)blockIdx.x * BN_PAIR_WG + threadIdx.x) >> 1;
  const bool live = i < n;
  const uint32_t* row = bits + (live ? i : 0) * bm_words;
  __shared__ G2Jac lds_acc[BN_PAIR_WG];
  static_assert(sizeof(G2Jac) == 3 * BN_LIMBS * 4, "accumulator: 27 words per lane in the pair layout");
  G2Jac& acc = lds_acc[threadIdx.x];
  if (rec) bm_sum_tables(acc, row, bm_words, live, K, rec, rec_inf);      // wave-uniform
  else bm_sum_keys(acc, row, bm_words, live, K);
  G2Affine pk;
  bm_sum_to_key(pk, acc);
  if (!live) return;
  ws_store_fp(ws, PL_QX0 + (int)role, i, pk.x.c[0]);
  ws_store_fp(ws, PL_QY0 + (int)role, i, pk.y.c[0]);
  if (role == 0) {
    const uint8_t prev = ws_byte(ws, BY_ST_DECODE, i);
    ws_byte(ws, BY_ST_DECODE, i) = prev != ST_OK ? prev : bm_rule2_status(row, bm_words, K);
    ws_byte(ws, BY_Q_INF, i) = pk.inf;
  }
}
int bn254_pair_bitmap_sum(const uint32_t* d_bits, size_t bm_words, size_t n, BmKeysArg keys, const int32_t* rec, const uint8_t* rec_inf, Ws ws, hipStream_t s) {
  const BmKeys K = {keys.xy, keys.st, keys.inf, keys.bad, keys.n_keys};
  k_bm_sum_pair<<<(unsigned)((2 * n + BN_PAIR_WG - 1) / BN_PAIR_WG), BN_PAIR_WG, 0, s>>>(d_bits, bm_words, n, K, rec, rec_inf, ws);
  HIP_TRY(hipGetLastError());
  return 0;
}
