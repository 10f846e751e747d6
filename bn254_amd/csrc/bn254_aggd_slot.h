// The slot helpers of the aggregates over distinct messages against registered keys, shared by the lane-pair translation units that run
// a table-driven slot kernel (bn254_aggkeyed.hip: the exact call; bn254_aggrand.hip: the randomised call's re-check).  Include after
// bn254_pairing.h and bn254_ws.h, with the defines of bn254_pair.hip.
#pragma once

struct Fp12PairSlot { Fp12 v; int32_t pad; };
static_assert(sizeof(Fp12PairSlot) == (6 * BN_LIMBS + 1) * 4 && ((6 * BN_LIMBS + 1) & 1), "LDS slot: 6 x 9 limbs + 1 pad word (odd stride: conflict-free)");

__device__ __forceinline__ Fp2 ws_load_fp2_own(const Ws& ws, int plane_re, size_t i) {
  Fp2 r;
  r.c[0] = ws_load_fp(ws, plane_re + (int)(threadIdx.x & 1u), i);
  return r;
}
__device__ __forceinline__ void ws_load_f12_own(const Ws& ws, size_t i, Fp12& f) {
  Fp2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
#pragma unroll
  for (int k = 0; k < 6; ++k) *c[k] = ws_load_fp2_own(ws, PL_F0 + 2 * k, i);
}
__device__ __forceinline__ void ws_store_f12_own(const Ws& ws, size_t i, const Fp12& f) {
  const Fp2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
#pragma unroll
  for (int k = 0; k < 6; ++k) ws_store_fp(ws, PL_F0 + 2 * k + (int)(threadIdx.x & 1u), i, c[k]->c[0]);
}

#include "bn254_aggd_reduce.h"

// ---- aggregates over distinct messages against REGISTERED keys (host side: bn254_aggdist.hip) -------------------------------------------
// Every G2 argument is a line table: aggregate i has k + 1 TABLE PAIRS, t < k: (H(m_{lo+t}) in the P1 planes at lo + t, lines of key
// key_idx[lo + t]), t = k: (sigma_i in the P1 planes at gbase + i, lines of -G2: the entry n_keys behind the registered keys).  Level 0:
// element e = SLOT e, the W table pairs W s .. W s + W - 1 of its aggregate (s = e minus the aggregate's first slot; a pair past k pads),
// through ONE Miller loop with no twist-point arithmetic (miller_loop_tables), then aggd_reduce as k_aggd_miller_pair.  Each lane pair
// reads its own points and table pointers (no branch on the pair's kind).  A refused or out-of-range key, an identity key or point and a
// padding pair are skipped pairs; the key-status kernel has recorded the refusals.  Needs n_keys > 0 (key 0 stands in for a refused key).
struct AggdTablePair { G1Affine p; const int32_t (*tab)[2][2][BN_LIMBS]; bool skip; };
__device__ __forceinline__ AggdTablePair aggd_table_pair(const Ws& ws, const uint32_t* key_idx, const KeyTable& kt, uint32_t seg, uint64_t lo, uint64_t k,
                                                         uint64_t t, size_t gbase) {
  typedef const int32_t (*LinePtr)[2][2][BN_LIMBS];
  const bool live = seg != AGGD_SEG_NONE, is_h = live && t < k;
  uint32_t key = kt.n_keys;                                         // -G2, also for padding and past the last slot
  bool skip = !live || t > k;
  if (is_h) {
    key = key_idx[lo + t];
    if (key >= kt.n_keys || kt.st[key] != ST_OK) { key = 0; skip = true; }
    else skip = kt.inf[key] != 0;
  }
  AggdTablePair r;
  ws_load_g1(ws, PL_P1X, BY_P1_INF, is_h ? (size_t)(lo + t) : gbase + (live ? seg : 0), r.p);
  r.skip = skip || r.p.inf;
  r.tab = (LinePtr)(kt.lines + (size_t)key * BN_N_FIXED_LINES * BN_KEY_LINE_WORDS);
  return r;
}
