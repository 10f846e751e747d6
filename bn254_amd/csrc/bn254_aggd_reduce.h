// The segmented product of the aggregate verify over distinct messages (bn254_aggdist.hip), shared by the lane-pair translation units that
// run its level-0 kernels (bn254_pair.hip: raw keys; bn254_aggkeyed.hip: registered keys).  Include after Fp12PairSlot, ws_store_f12_own and
// fp12_mul of the including unit.
#pragma once
// ELEMENTS, one per lane pair and AGGD_WG_ELEMS per workgroup, carry a segment id (the aggregate) and an Fq12 value.  Along the element
// array the ids of one aggregate are contiguous; AGGD_SEG_NONE marks elements of nobody (padding), which never take part in a product.
// aggd_reduce multiplies every run of equal ids by a tree aligned to the run's first element — round d: the element at run position r
// with r % 2d == 0 takes the product of the one d further on, if that is still in the run — 7 rounds of at most one fp12_mul per lane pair,
// the tree of the randomised kernels on the same representation (an operand is never rewritten in the round that reads it, so the product
// reads LDS in place).  Afterwards the first element of every run holds the run's product.
// A run that neither starts the workgroup nor reaches its end is a whole aggregate: F at gbase + seg.  The first and the last run may go on
// in a neighbouring workgroup: they become the workgroup's two PARTIALS (workspace index pbase + 2 block and + 1, ids in pseg; the second
// is one when a single run covers the workgroup), which the next level reduces the same way.  last = 1: the launch is one workgroup and
// every run is whole.  Both lanes of a pair take every branch together (the ids are per pair).
__device__ __forceinline__ void aggd_reduce(Fp12PairSlot* lds_f, uint32_t* lds_seg, uint32_t seg, const Ws& ws, size_t gbase, size_t pbase, uint32_t* pseg,
                                            int last) {
  const unsigned pair = threadIdx.x >> 1, role = threadIdx.x & 1u;
  Fp12& f = lds_f[threadIdx.x].v;
  if (role == 0) lds_seg[pair] = seg;
  __syncthreads();
  unsigned head = 0, hi = pair;                      // the first element of this run (the ids of a run are contiguous)
  while (head < hi) {
    const unsigned mid = (head + hi) >> 1;
    if (lds_seg[mid] == seg) hi = mid; else head = mid + 1;
  }
  const unsigned r = pair - head;
  for (unsigned d = 1; d < AGGD_WG_ELEMS; d <<= 1) {
    if (seg != AGGD_SEG_NONE && (r & (2 * d - 1)) == 0 && pair + d < AGGD_WG_ELEMS && lds_seg[pair + d] == seg)
      fp12_mul(f, f, lds_f[threadIdx.x + 2 * d].v);
    __syncthreads();
  }
  if (pair != 0 && lds_seg[pair - 1] == seg) return;   // not the head of its run
  const bool first = pair == 0, reaches_end = lds_seg[AGGD_WG_ELEMS - 1] == seg;
  if (last || (!first && !reaches_end)) {
    if (seg != AGGD_SEG_NONE) ws_store_f12_own(ws, gbase + seg, f);
    return;
  }
  const size_t p0 = pbase + 2 * (size_t)blockIdx.x;
  if (first) {
    ws_store_f12_own(ws, p0, f);
    if (role == 0) pseg[2 * (size_t)blockIdx.x] = seg;
    if (!reaches_end) return;
    fp12_set_one(f);                                 // one run covers the workgroup: the second partial is one
  }
  ws_store_f12_own(ws, p0 + 1, f);
  if (role == 0) pseg[2 * (size_t)blockIdx.x + 1] = seg;
}
