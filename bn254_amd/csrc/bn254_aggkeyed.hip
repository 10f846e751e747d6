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

#include "bn254_aggd_slot.h"
static inline unsigned aggd_grid(size_t n_elems) { return (unsigned)((n_elems + AGGD_WG_ELEMS - 1) / AGGD_WG_ELEMS); }

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
