// Translation unit of libbn254hip.so: KEY DEDUPLICATION of the exact verify (bn254_batch_verify_device on lane pairs).
//
// Pair A of a verify is e(H(m), pk); its twist-point walk (64 doublings, 23 additions: ~2.9 k of the 11.1 k Fq products of a verify's
// Miller loop) depends on pk alone.  A validator-set batch uses few keys many times, so the call finds its distinct keys and tabulates
// each one's 87 lines ONCE, in the exact format of bn254_ctx_register_keys (bn254_pairing.h: g2_line_table, c2 = 1, canonical limbs);
// k_miller_verify_keyed_pair then runs the loop on the tables.  All of it is enqueued on a stream of the context beside the decode and
// hash kernels of the call, and the route is decided ON THE DEVICE (no host sync):
//   k_kd_insert   one lane per item: open addressing over 2n+ slots keyed by a hash of the 32 words of the key, atomicCAS; two items share
//                 an entry only if all 128 bytes are equal (equal bytes decode equally, so grouping by bytes is exact).  The winner of a
//                 slot takes the next dense key id (atomicAdd) and records itself as the key's representative.  A probe sequence longer
//                 than KD_MAX_PROBES (an adversarial batch) sets KD_OVERFLOW: the call takes the generic route.
//   k_kd_match    THE KEY CACHE (BN254_OPT_KEY_CACHE): the tables are a pure function of a key's 128 bytes (and of the decode flags), and a validator
//                 set's keys are the same from call to call, so the rows of kd.lines / st / inf stay between calls.  One workgroup looks each
//                 of the call's D keys up in an index over the cached keys' bytes (kd.c_keys: the context's own copy; full 128-byte compare
//                 again); a hit takes its row, a miss the next free row, in the order of the ids, and goes on the build list.  Misses that do
//                 not fit the free rows drop the cache: the call builds all its keys into rows 0 .. D - 1, as a call without a cache does.
//                 A batch the thresholds refuse looks nothing up and leaves the cache alone.
//   k_kd_resolve  key_idx[i] = the ROW of the key of item i's slot
//   (the two builder kernels run over the build list only and leave at entry when it is empty)
//   k_kd_lines    one key on nine lane pairs, three keys per wave (bn254_kdlines.h: the lane machine's wave-T program, 204 product levels):
//                 decode of the representative (the statuses of the items themselves stay what launch_decode_g2 writes), the twist-point
//                 walk of g2_line_table with the RAW lines (c0, c1, c2) stored; a line with c2 = 0 (not reachable from the order-r subgroup,
//                 but keys are not subgroup-checked under flags = 0) sets KD_DEGENERATE.  No key bytes that reach such a line are known (the
//                 twist's order-10 069 points do not), so BN254_OPT_KEY_DEDUP_FORCE_GENERIC = 2 makes the builder report one for every key it builds
//   k_kd_scale    one workgroup per key, one lane pair per line: c0 / c2, c1 / c2, canonical — the values of g2_line_table's emit, so the
//                 tables are word for word those of registration; ONE inversion per key (a product tree over its 87 c2 in LDS).  Its tail
//                 folds the 22 places where two lines of the key meet with no squaring between them into rows of five coefficients
//                 (kd.fold; bn254_keydedup.h: kd_fold_pair), which k_miller_verify_keyed_fold_pair reads (BN254_OPT_KEY_DEDUP_FOLD)
//   k_kd_decide   the route: keyed iff D <= max_keys, D * min_multiplicity <= n, no overflow, no degenerate line; written as the device-side
//                 item counts the two Miller kernels read at entry (the unchosen one returns at once).  A keyed call COMMITS its build list to
//                 the cache here (index entries, rows in use); a generic one — forced, or a degenerate line among the keys it built —
//                 commits nothing, so a key with a degenerate line is never cached and the rows it wrote stay free.
#include <hip/hip_runtime.h>

#define BN_SPLIT_FP2 1
#define bn254 bn254_kd     // own namespace: the pair layout's types (bn254_fp2_pair.h)
#include "bn254_pairing.h"
#include "bn254_keydedup.h"
#include "bn254_lmachine.h"
#include "bn254_kdlines.h"

using namespace bn254;

#include "bn254_ws.h"

#define KD_WG 256
#define KERNEL_KD_PAIR __global__ __launch_bounds__(KD_WG) __attribute__((amdgpu_waves_per_eu(2, 2)))
#define KERNEL_KD __global__ __launch_bounds__(KD_WG)

__device__ __forceinline__ uint32_t kd_hash(const uint32_t* w, uint32_t hash_mask) {
  uint32_t h = 0x9E3779B9u;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    h ^= w[k];
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
  }
  h ^= h >> 16; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h & hash_mask;
}
__device__ __forceinline__ bool kd_same_key(const uint32_t* pks, uint32_t other, const uint32_t* w) {
  const uint32_t* o = pks + (size_t)other * 32;
  bool eq = true;
#pragma unroll
  for (int k = 0; k < 32; ++k) eq = eq && o[k] == w[k];
  return eq;
}
KERNEL_KD void k_kd_insert(const uint8_t* pks8, size_t n, KeyDedup kd) {
  const size_t i = (size_t)blockIdx.x * KD_WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t* pks = (const uint32_t*)pks8;           // 4-byte aligned (the entry point checks)
  uint32_t w[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) w[k] = pks[i * 32 + k];
  const uint32_t h = kd_hash(w, kd.hash_mask);
  for (uint32_t probe = 0; probe < KD_MAX_PROBES; ++probe) {
    const uint32_t s = (h + probe) & kd.slot_mask;
    uint32_t cur = __atomic_load_n(&kd.table[s], __ATOMIC_RELAXED);
    if (cur == KD_EMPTY) {
      cur = atomicCAS(&kd.table[s], KD_EMPTY, (uint32_t)i);
      if (cur == KD_EMPTY) {                                // this item represents a new key
        const uint32_t id = atomicAdd(&kd.ctl[KD_CTL_D], 1u);
        kd.slot_id[s] = id;
        if (id < kd.max_keys) kd.rep[id] = (uint32_t)i;
        kd.slot_of[i] = s;
        return;
      }
    }
    if (kd_same_key(pks, cur, w)) { kd.slot_of[i] = s; return; }   // full 128-byte compare: a hash match alone is not enough
  }
  kd.slot_of[i] = KD_EMPTY;
  atomicOr(&kd.ctl[KD_CTL_FLAGS], (uint32_t)KD_OVERFLOW);
}
// the table route is possible at all
__device__ __forceinline__ bool kd_viable(const KeyDedup& kd, size_t n) {
  const uint32_t d = kd.ctl[KD_CTL_D];
  return d <= kd.max_keys && (size_t)d * kd.min_mult <= n && (kd.ctl[KD_CTL_FLAGS] & KD_OVERFLOW) == 0;
}
// One workgroup: the call's keys against the cache.  The index holds COMMITTED rows only (k_kd_decide), c_state[0] of them; the rows from there
// on are free.  Rows are handed out by a prefix sum in the order of the ids, so a call into an empty cache gets row = id, the layout of a
// call without a cache.
#define KD_MATCH_WG 1024
__global__ __launch_bounds__(KD_MATCH_WG) void k_kd_match(const uint8_t* pks8, size_t n, KeyDedup kd, int reset) {
  __shared__ uint32_t scan[KD_MATCH_WG];
  __shared__ uint32_t s_misses;
  const uint32_t t = threadIdx.x;
  const uint32_t* pks = (const uint32_t*)pks8;
  if (reset) {
    for (uint32_t s = t; s <= kd.index_mask; s += KD_MATCH_WG) kd.c_index[s] = KD_EMPTY;
    if (t == 0) kd.c_state[0] = 0;
  }
  if (t == 0) s_misses = 0;
  __syncthreads();
  if (!kd_viable(kd, n)) {                                  // the generic route: nothing looked up, nothing built (KD_CTL_BUILD = KD_CTL_HITS = 0)
    if (t == 0) kd.ctl[KD_CTL_DROPPED] = reset ? (uint32_t)KD_DROP_RESET : 0u;
    return;
  }
  const uint32_t d = kd.ctl[KD_CTL_D];
  uint32_t used = reset ? 0u : kd.c_state[0];
  for (uint32_t id = t; id < d; id += KD_MATCH_WG) {
    uint32_t row = KD_EMPTY;
    if (used) {
      uint32_t w[32];
#pragma unroll
      for (int k = 0; k < 32; ++k) w[k] = pks[(size_t)kd.rep[id] * 32 + k];
      const uint32_t h = kd_hash(w, kd.hash_mask);
      for (uint32_t probe = 0; probe <= kd.index_mask; ++probe) {     // the index is at most half full: an empty slot ends every probe sequence
        const uint32_t r = kd.c_index[(h + probe) & kd.index_mask];
        if (r == KD_EMPTY) break;
        if (kd_same_key(kd.c_keys, r, w)) { row = r; break; }          // full 128-byte compare, as in k_kd_insert
      }
    }
    kd.row_of[id] = row;
    if (row == KD_EMPTY) atomicAdd(&s_misses, 1u);
  }
  __syncthreads();
  const bool drop = used + s_misses > kd.max_keys;          // the misses do not fit: drop the cache, build every key of the call (D <= max_keys)
  if (drop) {
    for (uint32_t s = t; s <= kd.index_mask; s += KD_MATCH_WG) kd.c_index[s] = KD_EMPTY;
    for (uint32_t id = t; id < d; id += KD_MATCH_WG) kd.row_of[id] = KD_EMPTY;
    if (t == 0) kd.c_state[0] = 0;
    used = 0;
  }
  uint32_t built = 0;                                       // misses among the ids below the current chunk (workgroup-uniform)
  for (uint32_t id0 = 0; id0 < d; id0 += KD_MATCH_WG) {
    const uint32_t id = id0 + t;
    const bool miss = id < d && kd.row_of[id] == KD_EMPTY;   // written by this very thread above
    scan[t] = miss ? 1u : 0u;
    __syncthreads();
    for (uint32_t o = 1; o < KD_MATCH_WG; o <<= 1) {         // inclusive prefix sum
      const uint32_t v = t >= o ? scan[t - o] : 0u;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    if (miss) {
      const uint32_t rank = built + scan[t] - 1, row = used + rank, item = kd.rep[id];
      kd.row_of[id] = row;
      kd.build_row[rank] = row;
      kd.build_rep[rank] = item;
#pragma unroll
      for (int k = 0; k < 32; ++k) kd.c_keys[(size_t)row * 32 + k] = pks[(size_t)item * 32 + k];   // the caller's buffer may be gone by the next call
    }
    built += scan[KD_MATCH_WG - 1];
    __syncthreads();
  }
  if (t == 0) {
    kd.ctl[KD_CTL_BUILD] = built;
    kd.ctl[KD_CTL_HITS] = d - built;
    kd.ctl[KD_CTL_DROPPED] = (drop ? (uint32_t)KD_DROP_CAPACITY : 0u) | (reset ? (uint32_t)KD_DROP_RESET : 0u);
  }
}
KERNEL_KD void k_kd_resolve(size_t n, KeyDedup kd) {
  const size_t i = (size_t)blockIdx.x * KD_WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = kd.slot_of[i];
  const uint32_t id = s == KD_EMPTY ? KD_EMPTY : kd.slot_id[s];
  const bool looked_up = kd.ctl[KD_CTL_BUILD] + kd.ctl[KD_CTL_HITS] != 0;   // k_kd_match wrote row_of (a batch the thresholds refuse: it did not)
  kd.key_idx[i] = looked_up && id < kd.max_keys ? kd.row_of[id] : 0u;        // (otherwise the call takes the generic route: nothing reads this)
}

__device__ __forceinline__ void kd_store_own(int32_t* dst, const Fp2& x) {
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) dst[(threadIdx.x & 1u) * BN_LIMBS + k] = x.c[0].v[k];
}
__device__ __forceinline__ Fp2 kd_load_own(const int32_t* src) {
  Fp2 r;
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) r.c[0].v[k] = src[(threadIdx.x & 1u) * BN_LIMBS + k];
  return r;
}
// The builder (bn254_kdlines.h): one key on nine lane pairs, three keys per wave, one wave per workgroup, so that the keys spread over CUs;
// per key and lane role a register file in LDS.  Every lane of a key decodes its representative (bn254_keydedup.h: decode_g2_pair_role,
// the decode of k_decode_g2_pair; no subgroup ladder); a refused key or the identity gets the generator's lines (its pair A is skipped).
// Then the lane machine's wave-T program: after each step pairs 0 / 1 / 2 store the RAW line's c0, c1 into the key's table row (scaled in
// place by k_kd_scale) and its c2 into kd.c2 (the head of the key's folded rows, which k_kd_scale writes last).  Lanes 54 .. 63 follow along on copies of the third key, without writing.
#define KD_LM_PER_WAVE 3                           // keys per wave
#define KD_LM_LANES 18                             // lanes per key: nine lane pairs
#define KD_LM_ROLE_STRIDE (LS_KD_SLOTS * BN_LIMBS + 1)
#define KD_LM_KEY_STRIDE (2 * KD_LM_ROLE_STRIDE)
#define KD_LM_LDS_WORDS (KD_LM_PER_WAVE * KD_LM_KEY_STRIDE)
static_assert(KD_LM_PER_WAVE * KD_LM_LANES <= BN_WAVE, "keys per wave");
#define KERNEL_KD_LM __global__ __launch_bounds__(BN_WAVE) __attribute__((amdgpu_waves_per_eu(1, 1)))
#define KD_LM_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

extern __shared__ int32_t kd_lds[];

struct KdLdsBox {
  typedef unsigned Ref;
  unsigned base;                 // word offset of slot 0 of the lane's key and role
  __device__ __forceinline__ Ref slot(uint32_t id) const { return base + id * BN_LIMBS; }
  __device__ __forceinline__ Fp2 get(Ref off) const {
    Fp2 r;
#pragma unroll
    for (int i = 0; i < BN_LIMBS; ++i) r.c[0].v[i] = kd_lds[off + i];
    return r;
  }
  __device__ __forceinline__ void put(Ref off, const Fp2& x) const {
#pragma unroll
    for (int i = 0; i < BN_LIMBS; ++i) kd_lds[off + i] = x.c[0].v[i];
  }
};
// the machine kd_builder_program drives, on the lanes of one key
struct KdLmDev {
  KdLdsBox bx;
  LmEntry e[KD_LV_N];            // this pair's entry of every level
  unsigned pair;
  bool writer, live, degenerate;
  int32_t* rows;
  int32_t* c2s;
  // products, publish, linear combinations, publish; a wave's LDS instructions execute in order, the fences keep the compiler's order
  __device__ __forceinline__ void level(int lv) {
    const LmEntry& en = e[lv];
    {
      const Fp2 pr = lm_stage_product(en, bx, 0);
      KD_LM_FENCE();
      if (writer && (en.w[1] & 255u) != (uint32_t)LS_DUMMY) bx.put(lm_product_out(en, bx, 0), pr);
      KD_LM_FENCE();
    }
    const Fp2 li = lm_stage_linear(en, bx, 0, false, false);
    KD_LM_FENCE();
    if (writer && (en.w[4] & 255u) != (uint32_t)LS_DUMMY) bx.put(lm_linear_out(en, bx, 0), li);
    KD_LM_FENCE();
  }
  __device__ __forceinline__ void add_point(int qx, int qy) {
    const Fp2 x = bx.get(bx.slot((uint32_t)qx)), y = bx.get(bx.slot((uint32_t)qy));
    if (writer) { bx.put(bx.slot(LS_TQX), x); bx.put(bx.slot(LS_TQY), y); }   // identical words from every pair of the key
    KD_LM_FENCE();
  }
  __device__ __forceinline__ void line(int idx, int kind) {
    degenerate = fp2_is_zero(bx.get(bx.slot((uint32_t)kd_line_slot(kind, 2)))) || degenerate;   // pair-combined: every lane
    const int c = pair < 3 ? (int)pair : 2;
    const Fp2 v = bx.get(bx.slot((uint32_t)kd_line_slot(kind, c)));
    if (live && pair < 3) kd_store_own(c == 2 ? c2s + (size_t)idx * 2 * BN_LIMBS : rows + (size_t)idx * BN_KEY_LINE_WORDS + (size_t)c * 2 * BN_LIMBS, v);
  }
};
KERNEL_KD_LM void k_kd_lines(const uint8_t* pks, uint32_t flags, KeyDedup kd, int report_degenerate) {
  const uint32_t d = kd.ctl[KD_CTL_BUILD];                                      // the build list (k_kd_match); 0 on the generic route
  if ((uint32_t)blockIdx.x * KD_LM_PER_WAVE >= d) return;                       // the whole wave leaves
  __builtin_amdgcn_s_setprio(3);                         // a latency chain beside the hash rounds' throughput waves
  const unsigned l = threadIdx.x, v = l / KD_LM_LANES, role = l & 1u;
  KdLmDev m;
  m.writer = v < KD_LM_PER_WAVE;
  const unsigned vslot = m.writer ? v : KD_LM_PER_WAVE - 1;
  m.pair = (l % KD_LM_LANES) >> 1;
  uint32_t j = (uint32_t)blockIdx.x * KD_LM_PER_WAVE + vslot;
  m.live = m.writer && j < d;
  if (j >= d) j = d - 1;                                 // lanes without a key of their own follow along on the last one
  const uint32_t row = kd.build_row[j];
  m.bx.base = vslot * KD_LM_KEY_STRIDE + role * KD_LM_ROLE_STRIDE;
  G2Affine q;
  const uint8_t st = decode_g2_pair_role(q, pks + 128 * (size_t)kd.build_rep[j], flags);
  const bool real = st == ST_OK && !q.inf;               // a refused key or the identity: generator lines (its pair A is skipped)
  if (!real) { q.x = fp2_load_const(C_G2_GEN[0]); q.y = fp2_load_const(C_G2_GEN[1]); }
  if (m.live && m.pair == 0 && role == 0) { kd.st[row] = st; kd.inf[row] = q.inf; }
  if (m.writer) {
    m.bx.put(m.bx.slot(LS_ZERO), fp2_zero()); m.bx.put(m.bx.slot(LS_DUMMY), fp2_zero());
    kd_builder_init(m.bx, q);
  }
#pragma unroll
  for (int lv = 0; lv < KD_LV_N; ++lv) {
    const LmEntry* t = kd_level_table(lv);
#pragma unroll
    for (int k = 0; k < 5; ++k) m.e[lv].w[k] = t[m.pair].w[k];
  }
  m.rows = kd.lines + (size_t)row * BN_N_FIXED_LINES * BN_KEY_LINE_WORDS;
  m.c2s = kd.c2 + (size_t)row * KD_FOLD_KEY_WORDS;
  m.degenerate = false;
  KD_LM_FENCE();
  kd_builder_program(m);
  if (m.live && ((real && m.degenerate) || report_degenerate) && m.pair == 0 && role == 0) atomicOr(&kd.ctl[KD_CTL_FLAGS], (uint32_t)KD_DEGENERATE);
}
// one workgroup per key, one lane pair per line: (c0, c1) <- canonical (c0 / c2, c1 / c2) with ONE inversion per key.  Montgomery's trick as a
// tree over the key's 87 c2 values (padded with ones to KD_TREE_LEAVES) in LDS — bn254_keydedup.h: kd_scale_tree is its host form —, heap order (node 1 = the root, leaves from KD_TREE_LEAVES on):
// seven product levels up, fp2_inv of the root, seven levels down (inverse of a node = inverse of its parent x its sibling), then the two
// products of kd_scale_line.  Field arithmetic is exact and the results are canonical, so the table words are those of kd_scale_line line by
// line.  A key with a line c2 = 0 has a zero root: every "inverse" is then what fp2_inv gives for zero times other values — finite work, no
// table anyone reads (k_kd_lines has set KD_DEGENERATE).
static_assert(BN_N_FIXED_LINES <= KD_TREE_LEAVES && 2 * KD_TREE_LEAVES == KD_WG, "one lane pair per leaf");
#define KD_NODE_WORDS (2 * BN_LIMBS)
KERNEL_KD_PAIR void k_kd_scale(KeyDedup kd) {
  if (blockIdx.x >= kd.ctl[KD_CTL_BUILD]) return;                  // the whole workgroup leaves
  const uint32_t j = kd.build_row[blockIdx.x];                     // the row of this key's table
  __shared__ int32_t prod[2 * KD_TREE_LEAVES * KD_NODE_WORDS];     // products of the subtrees
  __shared__ int32_t inv[2 * KD_TREE_LEAVES * KD_NODE_WORDS];      // ... and their inverses
  const uint32_t p = threadIdx.x >> 1;
  const bool line = p < BN_N_FIXED_LINES;
  int32_t* row = kd.lines + ((size_t)j * BN_N_FIXED_LINES + (line ? p : 0u)) * BN_KEY_LINE_WORDS;
  {
    Fp2 leaf = fp2_one();
    if (line) leaf = fp2_reduce_weak(kd_load_own(kd.c2 + (size_t)j * KD_FOLD_KEY_WORDS + p * KD_NODE_WORDS));   // site 290's default, for the raw slot value
    kd_store_own(prod + (KD_TREE_LEAVES + p) * KD_NODE_WORDS, leaf);
  }
  __syncthreads();
  for (uint32_t w = KD_TREE_LEAVES / 2; w >= 1; w >>= 1) {          // nodes w .. 2w - 1
    if (p < w) {
      const uint32_t node = w + p;
      kd_store_own(prod + node * KD_NODE_WORDS, fp2_mul(kd_load_own(prod + 2 * node * KD_NODE_WORDS), kd_load_own(prod + (2 * node + 1) * KD_NODE_WORDS)));
    }
    __syncthreads();
  }
  if (threadIdx.x < BN_WAVE) {                                      // one wave inverts the root (every pair the same value; pair 0 publishes it)
    const Fp2 r = fp2_inv(kd_load_own(prod + KD_NODE_WORDS));
    if (p == 0) kd_store_own(inv + KD_NODE_WORDS, r);
  }
  __syncthreads();
  for (uint32_t w = 2; w <= KD_TREE_LEAVES; w <<= 1) {              // nodes w .. 2w - 1
    if (p < w) {
      const uint32_t node = w + p;
      kd_store_own(inv + node * KD_NODE_WORDS, fp2_mul(kd_load_own(inv + (node >> 1) * KD_NODE_WORDS), kd_load_own(prod + (node ^ 1u) * KD_NODE_WORDS)));
    }
    __syncthreads();
  }
  if (line) {
    const Fp2 c2inv = kd_load_own(inv + (KD_TREE_LEAVES + p) * KD_NODE_WORDS);
    const Fp2 a = fp2_mul(kd_load_own(row), c2inv), b = fp2_mul(kd_load_own(row + 2 * BN_LIMBS), c2inv);
    Fp2 r0, r1;
    BN_FOR_ROLES(k) { r0.c[k] = fp_canon(a.c[k]); r1.c[k] = fp_canon(b.c[k]); }
    kd_store_own(row, r0);
    kd_store_own(row + 2 * BN_LIMBS, r1);
    // ... and into the leaves of the two trees, which nobody reads any more (the last level down has passed its barrier; the leaf of `inv`
    // was this pair's own): the folded rows below take both lines of a row from there
    kd_store_own(prod + (KD_TREE_LEAVES + p) * KD_NODE_WORDS, r0);
    kd_store_own(inv + (KD_TREE_LEAVES + p) * KD_NODE_WORDS, r1);
  }
  __syncthreads();
  // THE FOLDED ROWS (bn254_keydedup.h: kd_fold_pair; host form kd_fold_lines): lane pair r < BN_N_FOLD_ROWS folds lines C_FOLD_FIRST[r] and the next
  if (p >= BN_N_FOLD_ROWS) return;
  const uint32_t first = C_FOLD_FIRST[p];
  Fp2 k[5];
  kd_fold_pair(kd_load_own(prod + (KD_TREE_LEAVES + first) * KD_NODE_WORDS), kd_load_own(inv + (KD_TREE_LEAVES + first) * KD_NODE_WORDS),
               kd_load_own(prod + (KD_TREE_LEAVES + first + 1) * KD_NODE_WORDS), kd_load_own(inv + (KD_TREE_LEAVES + first + 1) * KD_NODE_WORDS), k);
  int32_t* frow = kd.fold + (size_t)j * KD_FOLD_KEY_WORDS + p * BN_KEY_FOLD_WORDS;   // over the row's raw c2: every leaf was loaded before the first barrier
#pragma unroll
  for (int e = 0; e < 5; ++e) kd_store_own(frow + e * 2 * BN_LIMBS, k[e]);
}
KERNEL_KD void k_kd_decide(size_t n, KeyDedup kd, int force_generic, int cache_on) {
  const bool keyed = force_generic != 1 && kd_viable(kd, n) && (kd.ctl[KD_CTL_FLAGS] & KD_DEGENERATE) == 0;   // every lane the same
  if (threadIdx.x == 0) {
    kd.ctl[KD_CTL_KEYED_N] = keyed ? (uint32_t)n : 0u;
    kd.ctl[KD_CTL_GENERIC_N] = keyed ? 0u : (uint32_t)n;
  }
  if (!keyed || !cache_on) return;
  // commit: the keys this call built become findable; their rows follow the rows in use (k_kd_match handed them out from there)
  const uint32_t built = kd.ctl[KD_CTL_BUILD];
  for (uint32_t m = threadIdx.x; m < built; m += KD_WG) {
    const uint32_t row = kd.build_row[m];
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) w[k] = kd.c_keys[(size_t)row * 32 + k];
    const uint32_t h = kd_hash(w, kd.hash_mask);
    for (uint32_t probe = 0; probe <= kd.index_mask; ++probe)      // distinct keys, at most max_keys of them in 2 x max_keys slots or more
      if (atomicCAS(&kd.c_index[(h + probe) & kd.index_mask], KD_EMPTY, row) == KD_EMPTY) break;
  }
  if (threadIdx.x == 0) kd.c_state[0] += built;
}

int bn254_kd_enqueue(const uint8_t* d_pks, size_t n, uint32_t flags, KeyDedup kd, int force_generic, int cache_reset, int cache_on, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(kd.table, 0xFF, ((size_t)kd.slot_mask + 1) * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(kd.ctl, 0, KD_CTL_WORDS * sizeof(uint32_t), s));
  const unsigned g = (unsigned)((n + KD_WG - 1) / KD_WG);
  k_kd_insert<<<g, KD_WG, 0, s>>>(d_pks, n, kd);
  k_kd_match<<<1, KD_MATCH_WG, 0, s>>>(d_pks, n, kd, cache_reset || !cache_on);
  k_kd_resolve<<<g, KD_WG, 0, s>>>(n, kd);
  k_kd_lines<<<(unsigned)((kd.max_keys + KD_LM_PER_WAVE - 1) / KD_LM_PER_WAVE), BN_WAVE, KD_LM_LDS_WORDS * sizeof(int32_t), s>>>(d_pks, flags, kd, force_generic == 2);
  k_kd_scale<<<kd.max_keys, KD_WG, 0, s>>>(kd);
  k_kd_decide<<<1, KD_WG, 0, s>>>(n, kd, force_generic, cache_on);
  HIP_TRY(hipGetLastError());
  return 0;
}
