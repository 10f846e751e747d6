// Translation unit of libbn254hip.so: level 0 of the aggregate verify over distinct messages against REGISTERED keys on lane pairs
// (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed[_device]; host side: bn254_aggdist.hip).  Compiled with the defines of
// bn254_pair.hip, as bn254_fe.hip is, in a code object of its own: the kernels of bn254_pair.hip keep their code and their placement.
#include <hip/hip_runtime.h>

#define BN_SPLIT_FP2 1
#if defined(BN_PAIR_FP6_LAZY) && !defined(BN_FP6_LAZY)
#define BN_FP6_LAZY 1
#endif
#ifndef BN_PAIR_NO_SQR_DPP_ASM
#define BN_PAIR_SQR_DPP_ASM 1
#endif
#ifndef BN_PAIR_CALL_FP12_HOT
#define BN_INLINE_FP12_HOT 1
#endif
#ifndef BN_PAIR_CALL_MUL_LINE
#define BN_INLINE_MUL_LINE 1
#endif
#ifndef BN_PAIR_CALL_FE_HOT
#define BN_INLINE_FE_HOT 1
#endif
#ifndef BN_PRIO_SHIFT
#define BN_PRIO_SHIFT 1
#endif
#define BN_SET_STEP_PRIORITY(step)                                                        \
  do {                                                                                    \
    if (((step) & ((1 << BN_PRIO_SHIFT) - 1)) == 0) {                                     \
      int q_ = ((step) >> BN_PRIO_SHIFT) & 3;                                             \
      if (q_ == 0) __builtin_amdgcn_s_setprio(3);                                         \
      else if (q_ == 1) __builtin_amdgcn_s_setprio(2);                                    \
      else if (q_ == 2) __builtin_amdgcn_s_setprio(1);                                    \
      else __builtin_amdgcn_s_setprio(0);                                                 \
    }                                                                                     \
  } while (0)
#define bn254 bn254_aggk   // own namespace, as in bn254_fe.hip
#include "bn254_pairing.h"

using namespace bn254;

#include "bn254_ws.h"

#ifndef BN_PAIR_WG
#define BN_PAIR_WG 256
#endif
#define KERNEL_PAIR __global__ __launch_bounds__(BN_PAIR_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))

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
static inline unsigned aggd_grid(size_t n_elems) { return (unsigned)((n_elems + AGGD_WG_ELEMS - 1) / AGGD_WG_ELEMS); }

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
template <int W>
KERNEL_PAIR void k_aggd_keyed_pair(size_t n_slots, Ws ws, AggdSlots sl, const uint32_t* key_idx, KeyTable kt, size_t gbase, size_t pbase, uint32_t* pseg,
                                   int last) {
  const size_t e = ((size_t)blockIdx.x * BN_PAIR_WG + threadIdx.x) >> 1;
  const uint32_t seg = e < n_slots ? sl.slot_agg[e] : AGGD_SEG_NONE;   // no early return: every lane reaches the barriers
  uint64_t lo = 0, k = 0, t0 = 0;
  if (seg != AGGD_SEG_NONE) {
    lo = sl.lo[seg];
    k = sl.hi[seg] - lo;
    t0 = W * (e - (sl.incl[seg] - (k + W) / W));
  }
  const AggdTablePair a = aggd_table_pair(ws, key_idx, kt, seg, lo, k, t0, gbase);
  __shared__ Fp12PairSlot lds_f[BN_PAIR_WG];
  __shared__ uint32_t lds_seg[AGGD_WG_ELEMS];
  if constexpr (W == 2) {
    const AggdTablePair b = aggd_table_pair(ws, key_idx, kt, seg, lo, k, t0 + 1, gbase);
    miller_loop_tables<2, true>(lds_f[threadIdx.x].v, a.p, a.skip, a.tab, b.p, b.skip, b.tab);
  } else {
    miller_loop_tables<1, true>(lds_f[threadIdx.x].v, a.p, a.skip, a.tab, a.p, true, a.tab);
  }
  aggd_reduce(lds_f, lds_seg, seg, ws, gbase, pbase, pseg, last);
}
// the aggregate products and their status bytes from gbase + i to i, where the final exponentiation of a verify of n items reads them
// (after the last level: no slot reads the pair indices any more)
KERNEL_PAIR void k_aggd_move_pair(size_t n, Ws ws, size_t gbase) {
  const size_t i = ((size_t)blockIdx.x * BN_PAIR_WG + threadIdx.x) >> 1;
  if (i >= n) return;
  Fp12 f;
  ws_load_f12_own(ws, gbase + i, f);
  ws_store_f12_own(ws, i, f);
  if ((threadIdx.x & 1u) == 0) ws_byte(ws, BY_ST_DECODE, i) = ws_byte(ws, BY_ST_DECODE, gbase + i);
}
int bn254_pair_aggd_keyed(size_t n_slots, int width, Ws ws, AggdSlots sl, const uint32_t* key_idx, KeyTable kt, size_t gbase, size_t pbase, uint32_t* pseg,
                          int last, hipStream_t s) {
  if (width == 1) k_aggd_keyed_pair<1><<<aggd_grid(n_slots), BN_PAIR_WG, 0, s>>>(n_slots, ws, sl, key_idx, kt, gbase, pbase, pseg, last);
  else k_aggd_keyed_pair<2><<<aggd_grid(n_slots), BN_PAIR_WG, 0, s>>>(n_slots, ws, sl, key_idx, kt, gbase, pbase, pseg, last);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_pair_aggd_move(size_t n, Ws ws, size_t gbase, hipStream_t s) {
  k_aggd_move_pair<<<(unsigned)((2 * n + BN_PAIR_WG - 1) / BN_PAIR_WG), BN_PAIR_WG, 0, s>>>(n, ws, gbase);
  HIP_TRY(hipGetLastError());
  return 0;
}
