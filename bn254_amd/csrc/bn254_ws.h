// Workspace layout shared by the two device translation units of libbn254hip.so (bn254_hip.hip: one item per
// lane; bn254_pair.hip: one verify per lane PAIR).  Device-side only; include after the field headers.
#pragma once
#include <stddef.h>

#define BN_WAVE 64
#define BN_SPLIT_MAX_N ((size_t)98304)   // <= 1.5 waves per SIMD with one lane per verify
#define TRIO_MAX_BATCH_DEFAULT 16384               // octet layout up to TWO passes of one wave per SIMD (1024 SIMDs x 8 verifies): 3.5 ms at 8192, 6.5 ms at 16384 (lane pairs: 7.1 / 7.9 ms)
#define NONET_WIDE_MAX_BATCH 1024                  // ... and up to this size on EIGHTEEN lane pairs, one verify per wave: the 18 products of a multiplication in one round (0.63 -> 0.56 ms)
#define NONET_MAX_BATCH_DEFAULT 3072               // final exponentiation on nine lane pairs per verify up to this batch size: ONE pass of 3 verifies per wave on 1024 SIMDs (0.64 ms against the octet layout's 1.09; a second pass would cost 1.3)
#define LM_MAX_BATCH_DEFAULT 1536                   // Miller loop as the lane machine (bn254_lmiller.hip: nine lane pairs in each of four waves per verify, 3 verifies per workgroup, one workgroup per CU) up to this batch size: two passes over 256 CUs (0.43 ms one pass, 0.86 two; eight wave roles: 1.0); 0 = never
// ---- batch size -> kernel layout: the ONE routing table of the verify-shaped entry points ---------------------------------------------
// (verify, verify from compressed encodings, check_public_keys, aggregate verify's pairing part, keyed verify below its table route.)
// Four thresholds — the *_DEFAULT values above, overridden per context by BN254_OPT_LM_MAX_BATCH / _NONET_MAX_BATCH / _NONET_WIDE /
// _TRIO_MAX_BATCH — span the table; bn_route() is the only place that turns a batch size into layouts, bn_route_table() lists its rows
// (what bn254_debug_route_table hands to the tests, which generate every boundary +-1 from it instead of listing sizes by hand).
//   default rows:  n <=  1 024  lane machine      + eighteen lane pairs      (one verify per SIMD)
//                  n <=  1 536  lane machine      + nine lane pairs
//                  n <=  3 072  eight wave roles  + nine lane pairs
//                  n <= 16 384  eight wave roles  + octets
//                  above        lane pairs        + lane pairs               (two waves per SIMD: throughput)
enum BnMillerLayout { BN_ML_LANE_MACHINE = 0, BN_ML_WAVE_ROLES = 1, BN_ML_LANE_PAIRS = 2 };
enum BnFeLayout { BN_FE_NONET_WIDE = 0, BN_FE_NONET = 1, BN_FE_OCTET = 2, BN_FE_LANE_PAIRS = 3 };
struct BnRouteLimits { size_t lm_max, nonet_wide_max, nonet_max, small_max; };   // 0 = that layout is off; small_max bounds the whole small-batch family
struct BnRoute { int miller, fe; };
static inline BnRoute bn_route(const BnRouteLimits& L, size_t n) {
  BnRoute r = {BN_ML_LANE_PAIRS, BN_FE_LANE_PAIRS};
  if (n > L.small_max) return r;
  r.miller = n <= L.lm_max ? BN_ML_LANE_MACHINE : BN_ML_WAVE_ROLES;
  r.fe = n <= L.nonet_max ? (n <= L.nonet_wide_max ? BN_FE_NONET_WIDE : BN_FE_NONET) : BN_FE_OCTET;
  return r;
}
// rows (max_n[i], route[i]) in ascending order of max_n, the last one max_n = SIZE_MAX; returns the number of rows (<= 5)
static inline int bn_route_table(const BnRouteLimits& L, size_t* max_n, BnRoute* route, int cap) {
  size_t b[4] = {L.lm_max, L.nonet_wide_max, L.nonet_max, L.small_max};
  for (int i = 0; i < 4; ++i) if (b[i] > L.small_max) b[i] = L.small_max;
  for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j) if (b[j] < b[i]) { size_t t = b[i]; b[i] = b[j]; b[j] = t; }
  int rows = 0;
  for (int i = 0; i < 4 && rows < cap - 1; ++i) {
    if (b[i] == 0 || (i && b[i] == b[i - 1])) continue;
    const BnRoute r = bn_route(L, b[i]);
    if (rows && route[rows - 1].miller == r.miller && route[rows - 1].fe == r.fe) { max_n[rows - 1] = b[i]; continue; }
    max_n[rows] = b[i]; route[rows] = r; ++rows;
  }
  max_n[rows] = (size_t)-1; route[rows] = bn_route(L, (size_t)-1); ++rows;
  return rows;
}
#ifndef BN_WS_ROUTE_ONLY      /* (a host-side test includes the part above alone: tests/test_abi.py::test_routing_table_rows) */
#define TRIO_WAVE_ROLES_DEFAULT 2                  // ... with the Miller loop as wave roles: 2 = eight waves per 32 verifies (k_miller_verify_w8), 1 = four
#define AGG_SUBSET_MIN_TUPLES_DEFAULT 4096       // aggregate verify: subset-sum table of the key pool from this many tuples on (the table costs ~0.3 ms)
#define AGG_SUBSET_MAX_SIGNERS ((size_t)2048)     // ... one mask byte per group of 8 keys and tuple in LDS: 256 groups at most
#define AGG_SUBSET_G1_TUPLES_PER_MSG ((size_t)64)  // ... signature tables (per message) once a message is shared by this many tuples on average
#define AGG_SUBSET_G1_MAX_BYTES ((size_t)8 << 30)  // ... and while they stay below 8 GB of HBM
#define AGG_WIDE_MIN_TUPLES_DEFAULT 262144         // ... tables of twice the window (keys: 16 signers per entry, signatures: 8) from this many tuples on: half the additions
                                                   //     per tuple for ~6 ms of table building per call (k_pool_widen_g2 / _g1); 0 = never
#define AGG_WIDE_G1_TUPLES_PER_MSG ((size_t)512)   // ... the signature half only when a message's (16 x larger) table is shared by this many tuples
#define AGG_WIDE_G2_MAX_BYTES ((size_t)2 << 30)    // ... and the tables stay below these budgets of HBM
#define PINNED_STAGING_DEFAULT 0                    // host-pointer verify: threads copying through the pinned staging buffer; 0 = off (A/B in profiles/r04_*)
#define PINNED_STAGING_MIN_N ((size_t)8192)        // ... only batches whose transfer is worth overlapping
#define RAND_MIN_BATCH_DEFAULT 131072              // randomised verify pays off from about here
#define RAND_TWO_PER_LANE_MIN_N ((size_t)131072)   // randomised verify: two items per lane once that still fills 1024 SIMDs
// aggregate verify over distinct messages (bn254_aggdist.hip): a 256-lane workgroup reduces 128 ELEMENTS (one per lane pair) by a segmented
// product in LDS; the Miller kernel's elements are SLOTS of two pairs of one aggregate, so one workgroup takes up to AGGD_WG_PAIRS pairs
#define AGGD_WG_ELEMS 128
#define AGGD_WG_PAIRS 256
#define AGGD_TWO_PER_PAIR_MIN_M 131072            // ... two pairs per lane pair (shared squarings) from this many pairs on: below, m / 2 lane pairs leave the
                                                   //     1024 SIMDs at less than two waves each, and one pair per lane pair (k_miller_var_pair) is faster
#define AGGD_SEG_NONE 0xFFFFFFFFu                  // segment id of an element that belongs to no aggregate (padding, gaps between ranges)
// Register budget: amdgpu_waves_per_eu(W, W) on the kernels is propagated to every device function
// they call (AMDGPU attributor), capping VGPR+AGPR at 512/W so that W waves fit on each SIMD.
// In a pure-VALU microbenchmark two co-resident waves each keep the full single-wave issue rate
// (profiles/r01_issue_mix_microbench.jsonl), but the Fq12 bodies need ~400 live registers: at W = 2
// they spill to the private segment and every kernel got slower (profiles/r01_c_ab_occupancy.log).
// W = 1 (512 registers per lane) is the measured optimum for this code shape.
#ifndef BN_WAVES_PER_EU
#define BN_WAVES_PER_EU 1
#endif
#define KERNEL __global__ __launch_bounds__(BN_WAVE) __attribute__((amdgpu_waves_per_eu(BN_WAVES_PER_EU, BN_WAVES_PER_EU)))
// kernels whose per-lane state is a few field elements (hash rounds, decoders, encoders) fit 256
// registers without spilling and gain from a second wave per SIMD (hash: 1.34 -> 1.15 ms per 65 536)
#define KERNEL_SMALL __global__ __launch_bounds__(BN_WAVE) __attribute__((amdgpu_waves_per_eu(2, 2)))

// ------------------------------------------------------------------------------------------
// workspace planes
// ------------------------------------------------------------------------------------------
struct Ws {
  int32_t* planes;    // [N_PLANES * BN_LIMBS][stride] i32
  uint8_t* bytes;     // [N_BYTE_PLANES][stride]
  size_t stride;
  // hash-to-G1 round state (see k_hash_round)
  uint32_t* h_best;   // [stride]  smallest successful counter of the current round, or HASH_NONE
  uint8_t* h_next;    // [stride]  first counter not yet tried
  uint32_t* h_list;   // [2][stride] compacted indices of the messages still without a point
  uint32_t* h_cnt;    // [HASH_MAX_ROUNDS + 1] number of entries of the list feeding round r
  // clock probe (BN254_OPT_CLOCK_PROBE; nullptr = off): [3 slots: Miller loop, final exponentiation, probes][BN_CLK_MAX_WG][2] — per workgroup
  // index the shader-clock cycles (s_memtime) and the constant-rate ticks (s_memrealtime) its first lane saw between entry and exit,
  // ACCUMULATED over every launch since bn254_ctx_last_clocks last read (and cleared) them: their ratio is the clock the chip actually
  // ran those kernels at — over exactly the launches in between, e.g. the timed steps of bench.py (roofline.effective_sclk_mhz)
  unsigned long long* clk;
};
#define BN_CLK_MAX_WG 4096
#define BN_CLK_BEGIN(ws)                                                                         \
  unsigned long long clk0_ = 0, wall0_ = 0;                                                      \
  if ((ws).clk && threadIdx.x == 0) { clk0_ = clock64(); wall0_ = wall_clock64(); }
#define BN_CLK_END(ws, slot)                                                                     \
  do {                                                                                           \
    if ((ws).clk && threadIdx.x == 0 && blockIdx.x < BN_CLK_MAX_WG) {                            \
      unsigned long long* p_ = (ws).clk + ((size_t)(slot) * BN_CLK_MAX_WG + blockIdx.x) * 2;    \
      p_[0] += clock64() - clk0_; p_[1] += wall_clock64() - wall0_;                              \
    }                                                                                            \
  } while (0)
#define HASH_NONE 0xFFFFFFFFu
#define HASH_DONE 0xFFFFFFFEu                    // k_hash_direct has already written the point of this message
#define HASH_TAIL 0xFFFFFFFDu                    // a survivor of the wide schedule's round: a tail block of k_hash_finish_tail writes its point
#define HASH_DIRECT_WIDTH_DEFAULT 32             // counters tried at once per message by k_hash_direct (lanes of one wave; 1, 2, .. 32)
#define HASH_DIRECT_MAX_N ((size_t)4096)         // ... for batches that leave the chip mostly idle: 32 n lanes <= two waves per SIMD
#define HASH_MAX_ROUNDS 64
#define HASH_MAX_GRID_LANES ((size_t)1 << 24)   // lanes launched per round at most (grid-stride beyond)
#ifndef HASH_TARGET_LANES
#define HASH_TARGET_LANES ((size_t)1 << 17)    // ~2 waves per SIMD
#endif
// the wide schedule (launch_hash_rounds: one wide filter round, then finish and tail in one launch) from above HASH_DIRECT_MAX_N up to here;
// above, the multi-round schedule, which is throughput-bound there
#ifndef HASH_WIDE_MAX_N
#define HASH_WIDE_MAX_N ((size_t)32768)
#endif
#define HASH_WIDE_WAVES 1024                    // ... whose round is as wide as keeps finish and tail waves together below this (one wave per SIMD)
#define HASH_TAIL_CHUNK_DEFAULT 32              // counters a survivor's lane group tries at once in the tail (a power of two, 2 .. 32)
#define HASH_TAIL_MAX_BLOCKS ((size_t)16384)    // tail waves launched at most (the groups stride over the survivor list beyond)
enum { PL_P1X = 0, PL_P1Y, PL_QX0, PL_QX1, PL_QY0, PL_QY1, PL_P2X, PL_P2Y, PL_HASHX, PL_HASHY, PL_F0, N_PLANES = PL_F0 + 12 };
enum { BY_ST_DECODE = 0, BY_ST_HASH, BY_P1_INF, BY_Q_INF, BY_P2_INF, BY_A_INF, N_BYTE_PLANES };

__device__ __forceinline__ Fp ws_load_fp(const Ws& ws, int plane, size_t i) {
  Fp r;
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) r.v[k] = ws.planes[((size_t)plane * BN_LIMBS + k) * ws.stride + i];
  return r;
}
__device__ __forceinline__ void ws_store_fp(const Ws& ws, int plane, size_t i, const Fp& a) {
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) ws.planes[((size_t)plane * BN_LIMBS + k) * ws.stride + i] = a.v[k];
}
__device__ __forceinline__ uint8_t& ws_byte(const Ws& ws, int plane, size_t i) { return ws.bytes[(size_t)plane * ws.stride + i]; }

__device__ __forceinline__ void ws_store_g1(const Ws& ws, int px, int inf_plane, size_t i, const G1Affine& p) {
  ws_store_fp(ws, px, i, p.x); ws_store_fp(ws, px + 1, i, p.y); ws_byte(ws, inf_plane, i) = p.inf;
}
__device__ __forceinline__ void ws_load_g1(const Ws& ws, int px, int inf_plane, size_t i, G1Affine& p) {
  p.x = ws_load_fp(ws, px, i); p.y = ws_load_fp(ws, px + 1, i); p.inf = ws_byte(ws, inf_plane, i) != 0;
}

// Pools (aggregate verify) are decoded once into RECORDS: everything one lane reads of an entry is contiguous, because the
// aggregation kernels GATHER entries by index — with the limb-major planes of the workspace a point cost 18 cache lines per
// lane (1 152 distinct lines per wave-load, more than the L1 holds), with records it costs one or two.
//   G1 entry (2 coordinates):  [x (9 words) | y (9) | 2 pad]                                   = 20 words (80 B, 16-byte aligned)
//   G2 entry (4 coordinates):  [x.re (9) | y.re (9) | 2 pad] [x.im (9) | y.im (9) | 2 pad]     = 40 words: a lane of the pair
//                              layout reads the half of its role
// coordinate index e as before: G1 0 = x, 1 = y; G2 0 = x.re, 1 = x.im, 2 = y.re, 3 = y.im.  Status byte per entry.
#define BN_POOL_HALF_WORDS 20
struct Pool { int32_t* planes; uint8_t* st; size_t stride; uint32_t g2; };
__device__ __forceinline__ size_t pool_word(const Pool& p, int e, size_t j) {
  return p.g2 ? j * (2 * BN_POOL_HALF_WORDS) + (size_t)((e & 1) * BN_POOL_HALF_WORDS + (e >> 1) * BN_LIMBS) : j * BN_POOL_HALF_WORDS + (size_t)(e * BN_LIMBS);
}
__device__ __forceinline__ Fp pool_load_fp(const Pool& p, int e, size_t j) {
  Fp r;
  const int32_t* w = p.planes + pool_word(p, e, j);
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) r.v[k] = w[k];
  return r;
}
__device__ __forceinline__ void pool_store_fp(const Pool& p, int e, size_t j, const Fp& a) {
  int32_t* w = p.planes + pool_word(p, e, j);
#pragma unroll
  for (int k = 0; k < BN_LIMBS; ++k) w[k] = a.v[k];
}
#define HIP_TRY(expr)                                      \
  do {                                                     \
    hipError_t e_ = (expr);                                \
    if (e_ != hipSuccess) return -(int)e_;                 \
  } while (0)

// entry points of bn254_pair.hip (internal to the library)
__attribute__((visibility("hidden"))) int bn254_pair_miller_verify(size_t n, Ws ws, const uint32_t* map, const uint32_t* count, hipStream_t s,
                                                                   int mode = 0);
__attribute__((visibility("hidden"))) int bn254_pair_miller_var(size_t n, Ws ws, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_leaf_floor(size_t n, Ws ws, hipStream_t s, int mode);
__attribute__((visibility("hidden"))) int bn254_pair_fe_program(size_t n, Ws ws, const unsigned char* prog, hipStream_t s);   // measurement only      // measurement only
__attribute__((visibility("hidden"))) int bn254_pair_final_exp_product(size_t n, size_t k, Ws ws, uint8_t* gt_out, uint8_t* status_out, int raw_only,
                                                                       hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_final_exp(size_t n, Ws ws, int use_hash, uint8_t* status_out, const uint32_t* map,
                                                               const uint32_t* count, hipStream_t s, size_t base = 0);
__attribute__((visibility("hidden"))) int bn254_pair_miller_rand(size_t n, size_t n_groups, int items_per_pair, Ws ws, size_t gbase, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_rand_tail(size_t n_groups, Ws ws, size_t gbase, hipStream_t s);
// aggregate verify over distinct messages (bn254_aggdist.hip): the segmented Miller kernel (level 0 over slots), the generic level kernel over
// (segment, value) elements, and the sigma tail F_i * miller(sigma_i, -G2) from workspace index gbase + i to obase + i
struct AggdSlots { const uint32_t* slot_agg; const uint64_t* incl; const uint64_t* lo; const uint64_t* hi; };   // slot -> aggregate; per aggregate the inclusive
                                                                                                                // scan of its slot counts ceil((hi - lo) / 2) and its pair range [lo, hi)
__attribute__((visibility("hidden"))) int bn254_pair_aggd_miller(size_t n_slots, Ws ws, AggdSlots sl, size_t gbase, size_t pbase, uint32_t* pseg, int last,
                                                                 hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_aggd_level(size_t n_elems, Ws ws, const uint32_t* seg, size_t ebase, size_t gbase, size_t pbase,
                                                                 uint32_t* pseg, int last, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_aggd_tail(size_t n, Ws ws, size_t gbase, size_t obase, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_aggregate(const uint32_t* tuple_msg, const uint64_t* tuple_off, const uint32_t* signer_idx, size_t n,
                                                               size_t n_signers, size_t n_msgs, Pool pk_pool, Pool sig_pool, Pool h_pool, Pool sub_pool,
                                                               size_t n_groups, Pool sub1_pool, size_t groups4, Ws ws, hipStream_t s,
                                                               const uint32_t* perm = nullptr, const Pool* wide2_pool = nullptr,
                                                               const Pool* wide1_pool = nullptr);
__attribute__((visibility("hidden"))) int bn254_pair_g2_mul_fixed(const uint8_t* d_scalars, size_t n, int reduce, Pool comb, uint8_t* d_out, uint8_t* d_status,
                                                                  hipStream_t s);      // sk * G2::one() from the comb table of the generator (520 + 1 records)
#define BN_G2_COMB_RECORDS (65 * 8 + 1)
__attribute__((visibility("hidden"))) int bn254_pair_g1_mul_fixed(const uint8_t* d_scalars, size_t n, int reduce, Pool comb, uint8_t* d_out, uint8_t* d_status,
                                                                  hipStream_t s);      // sk * G1::one(): 520 records + the two blinding points + minus their sum
#define BN_G1_COMB_RECORDS (65 * 8 + 3)
__attribute__((visibility("hidden"))) int bn254_pair_decode_g2(const uint8_t* pts, size_t n, uint32_t flags, Ws ws, int accumulate, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_decompress_g2(const uint8_t* in, size_t n, Ws ws, hipStream_t s, int skip_subgroup_test = 0);

// keyed verify: the registered keys of a context — per key the 87 lines of its Miller loop in the c2 = 1 form,
// lines[key][line][coefficient c0 / c1][re / im][limb] (canonical limbs; 12.5 KB per key), its decode status and identity flag
#define BN_KEY_LINE_WORDS (2 * 2 * BN_LIMBS)
struct KeyTable { const int32_t* lines; const uint8_t* st; const uint8_t* inf; uint32_t n_keys; };
__attribute__((visibility("hidden"))) int bn254_lm_miller_verify_keyed(size_t n, Ws ws, const uint32_t* key_idx, KeyTable kt, hipStream_t s);   // bn254_lmiller.hip: the smallest batches
__attribute__((visibility("hidden"))) int bn254_pair_miller_verify_keyed(size_t n, Ws ws, const uint32_t* key_idx, KeyTable kt, hipStream_t s, size_t base = 0,
                                                                         const uint32_t* map = nullptr, const uint32_t* count = nullptr);
// ... on the folded rows of the key dedup (kd.fold: per key BN_N_FOLD_ROWS x (K0 .. K4) x (re, im) x limbs; bn254_pairing.h: miller_loop_keyed_fold)
#define BN_KEY_FOLD_WORDS (5 * 2 * BN_LIMBS)
__attribute__((visibility("hidden"))) int bn254_pair_miller_verify_keyed_fold(size_t n, Ws ws, const uint32_t* key_idx, KeyTable kt, const int32_t* fold,
                                                                              hipStream_t s, size_t base = 0, const uint32_t* map = nullptr,
                                                                              const uint32_t* count = nullptr);
// ... on the plain rows, the two unit lines of a step multiplied into f one at a time (bn254_pairing.h: miller_loop_keyed_unit)
__attribute__((visibility("hidden"))) int bn254_pair_miller_verify_keyed_unit(size_t n, Ws ws, const uint32_t* key_idx, KeyTable kt, hipStream_t s, size_t base = 0,
                                                                              const uint32_t* map = nullptr, const uint32_t* count = nullptr);
// aggregates over distinct messages against registered keys (bn254_aggdist.hip): level 0 over slots of `width` (1 or 2) table pairs whose
// per-aggregate inclusive slot scan is sl.incl (ceil((hi - lo + 1) / width)); the registered table holds -G2's lines as entry kt.n_keys.
// Then the aggregates' products from gbase + i to i for the final exponentiation.
#define AGGD_KEYED_W1_MAX_SLOTS 65536             // one table pair per lane pair while that needs at most this many lane pairs (one pass at 2 waves
                                                   // per SIMD: 16 384 x 4 takes 8.9 ms at width 1 against 6.9 at width 2, 1 024 x 4 3.2 against 3.8)
__attribute__((visibility("hidden"))) int bn254_pair_aggd_keyed(size_t n_slots, int width, Ws ws, AggdSlots sl, const uint32_t* key_idx, KeyTable kt,
                                                                size_t gbase, size_t pbase, uint32_t* pseg, int last, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_aggd_move(size_t n, Ws ws, size_t gbase, hipStream_t s);
// ... randomised (bn254_aggrand.hip; host side: bn254_aggdist.hip): the G1 side — groups, scaled entries, buckets, their segmented sums — and
// the exact slot kernel restricted to the aggregates marked in `queued` (null: every aggregate; a workgroup with none leaves before its Miller loop)
#define AGG_RAND_MIN_PAIRS_DEFAULT 65536           // BN254_OPT_AGG_RAND_MIN_PAIRS: the randomised call from this many messages on
#define AGG_RAND_GROUP_PAIRS_DEFAULT 1024          // BN254_OPT_AGG_RAND_GROUP_PAIRS: messages per group (at least the number of keys)
#define AGGR_SUM_WG 256                            // segmented G1 sums: elements (lanes) per workgroup
#define AGGR_PART_WORDS (3 * BN_LIMBS)             // ... a partial sum: one Jacobian point
struct AggrScale { const uint32_t* pair_agg; const uint32_t* key_idx; const uint8_t* key_inf; const uint64_t* lo; uint32_t* nagg; uint32_t* ebkt;
                   uint64_t* cnt; uint64_t G; uint32_t n_keys; };
struct AggrSum { const uint32_t* perm; const uint64_t* tp; uint32_t* bkey; size_t m, gbase, cbase, tbase; uint32_t n_keys; };
__attribute__((visibility("hidden"))) int bn254_aggr_scale(size_t m, size_t n, Ws ws, size_t gbase, AggrScale a, const uint32_t* seed_be, int mode,
                                                           hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_aggr_scatter(size_t n_entries, const uint32_t* ebkt, uint64_t* start, uint32_t* perm, uint32_t* eseg,
                                                             size_t n_b, uint32_t n_keys, const uint64_t* cnt, uint64_t* tp, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_aggr_glimits(size_t n_groups, uint32_t n_keys, size_t tbase, const uint64_t* cnt, const uint64_t* tp,
                                                             uint64_t* glo, uint64_t* ghi, Ws ws, size_t cbase, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_aggr_sum(size_t n_elems, int level0, Ws ws, AggrSum a, const uint32_t* seg_in, const int32_t* part_in,
                                                         uint32_t* pseg_out, int32_t* part_out, int last, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_aggr_collect(size_t n, Ws ws, size_t gbase, const uint64_t* lo, uint64_t G, const uint32_t* nagg,
                                                             const uint8_t* gst, uint8_t* status, uint8_t* queued, size_t n_groups, const uint64_t* glo,
                                                             const uint64_t* ghi, uint32_t* stats, hipStream_t s);
__attribute__((visibility("hidden"))) int bn254_pair_aggd_keyed_queued(size_t n_slots, int width, Ws ws, AggdSlots sl, const uint32_t* key_idx, KeyTable kt,
                                                                       size_t gbase, size_t pbase, uint32_t* pseg, int last, const uint8_t* queued,
                                                                       hipStream_t s);

// same-message aggregates given as signer bitmaps over the registered keys (bn254_bitmap.hip; lane pairs: bn254_bitmap_pair.hip; the walk:
// bn254_bitmap.h): tuple i's aggregate key from its bm_words bitmap words into the Q planes at index i, rule 2's status behind the
// signature's in BY_ST_DECODE.  rec / rec_inf = the subset tables of the registered set, or null: key by key from keys.xy
#define BITMAP_TABLE_MAX_KEYS_DEFAULT 4096         // BN254_OPT_BITMAP_TABLE_MAX_KEYS: subset tables while the set has at most this many keys (5 152 B per key: 21 MB)
struct BmKeysArg { const int32_t* xy; const uint8_t* st; const uint8_t* inf; const uint32_t* bad; uint32_t n_keys; };
__attribute__((visibility("hidden"))) int bn254_pair_bitmap_sum(const uint32_t* d_bits, size_t bm_words, size_t n, BmKeysArg keys, const int32_t* rec,
                                                                const uint8_t* rec_inf, Ws ws, hipStream_t s);

// ... randomised (bn254_bitmap_rand.hip), with two host helpers of bn254_aggdist.hip: the device-side prefix sum, and the slots
// of the slot kernel over n groups of table pairs [lo, hi) (count, scan, map)
#define BITMAP_RAND_MIN_TUPLES_DEFAULT 81920       // BN254_OPT_BITMAP_RAND_MIN_TUPLES: the randomised route from this many tuples on (measured: DESIGN.md §10d)
#define BITMAP_RAND_MAX_KEYS_DEFAULT 256           // BN254_OPT_BITMAP_RAND_MAX_KEYS: ... while the set has at most this many keys (its sums grow with n_keys / 8 per
                                                   //     tuple: at 1 024 keys it loses at every size measured)
#define BITMAP_RAND_GROUP_TUPLES_DEFAULT 4096      // BN254_OPT_BITMAP_RAND_GROUP_TUPLES: tuples per group of its combined checks (the sweeps at 65 536 and 2^20 x 256)
#define COLLECT_WAVE_MIN_SHARES_DEFAULT 16         // BN254_OPT_COLLECT_WAVE_MIN_SHARES (bn254_collect.hip): tuples with at least this many shares are summed by a
                                                   //     wave each, the shorter ones by a lane each — swept at three shapes only
#define POLY_EVAL_WAVE_MIN_COEFFS_DEFAULT 16       // BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS (bn254_polyeval.hip): polynomials with at least this many coefficients are
                                                   //     evaluated by a wave each, the shorter ones by a lane each — swept: 8 stays with the lanes, 16 ties or wins in waves
#define COLLECT_RAND_MIN_SHARES_DEFAULT 65664     // BN254_OPT_COLLECT_RAND_MIN_SHARES: bn254_batch_collect_keyed_bitmap_randomized groups the shares from this many on
                                                   //     (the smallest measured size at which it wins; at 45 056 shares it ties or loses: DESIGN.md §10f)
#define COLLECT_RAND_MIN_PER_KEY_DEFAULT 42        // BN254_OPT_COLLECT_RAND_MIN_PER_KEY: ... and from this many shares per registered key on (the smallest measured
                                                   //     ratio at which it wins; at 10 per key it loses, nothing measured in between)
#define COLLECT_OPT_MIN_SHARES_DEFAULT 1539        // BN254_OPT_COLLECT_OPT_MIN_SHARES: bn254_batch_collect_keyed_bitmap_optimistic checks sums from this many shares
                                                   //     on (the smallest measured size from which it wins, tuples of 171 shares: 1 026 ties, 513 loses)
#define COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT 1     // BN254_OPT_COLLECT_OPT_MIN_TUPLE_SHARES: ... and only the tuples with at least this many candidates.  1 = every
                                                   //     tuple: a tuple sent the exact way costs the call one pass of the queue's kernels, 4.9 ms measured whatever
                                                   //     the queue's length, and the check of a short tuple's sum costs nothing measurable
#define MERGE_WAVE_MIN_PARTS_DEFAULT 16            // BN254_OPT_MERGE_WAVE_MIN_PARTS (bn254_merge.hip): tuples with at least this many partials are merged by a
                                                   //     wave each.  Swept over 4 .. 256 partials at rows of 8 and of 128 words: the layouts
                                                   //     cross between 16 and 32 partials at 8 words, at 8 at 128 words; 16 has the smallest worst loss (0.15 ms)
#define THRESHOLD_OPT_MIN_SHARES_DEFAULT 513      // BN254_OPT_THRESHOLD_OPT_MIN_SHARES: bn254_batch_threshold_combine_keyed_optimistic checks results from this many
                                                   //     shares on (the smallest measured size, 3 x 171 shares: 3.81 ms against 4.03, beyond the exact call's spread; no
                                                   //     size measured loses with every share valid, nothing below 513 was measured)
#define MERGE_OPT_MIN_PARTS_DEFAULT 64             // BN254_OPT_MERGE_OPT_MIN_PARTS: bn254_batch_merge_keyed_bitmap_optimistic checks sums from this many partials
                                                   //     on (the smallest measured size from which it wins beyond the spread, tuples of 16 partials: 4 x 16 wins
                                                   //     by 3 %, 2 x 16 and 1 x 16 tie; nothing measured between 32 and 64)
__attribute__((visibility("hidden"))) int bn254_aggd_scan_add(hipStream_t s, const uint64_t* in, size_t n, uint64_t* out, uint64_t* tot);
__attribute__((visibility("hidden"))) int bn254_aggd_scan_max(hipStream_t s, const uint64_t* in, size_t n, uint64_t* out, uint64_t* tot);   // ... the prefix maximum
__attribute__((visibility("hidden"))) int bn254_aggd_keyed_slot_map(hipStream_t s, size_t n, const uint64_t* lo, const uint64_t* hi, int width,
                                                                    uint64_t* kincl, uint64_t* tot, size_t n_slots, uint32_t* slot_agg);

// key deduplication of the exact verify (bn254_keydedup.hip): per call, the distinct keys of the batch and their line tables in the
// KeyTable format above, built on a stream of the context beside decode and hash; the route (tables or the generic loop) is decided on the device
#define KEY_DEDUP_MAX_KEYS_DEFAULT 1024            // tables for at most this many distinct keys per call (12.5 KB + 7.9 KB of folded rows, which a key's raw c2 shares while it is built)
#define KEY_DEDUP_MIN_MULT_DEFAULT 16              // ... and only when every key serves this many items on average
#define KEY_DEDUP_FOLD_DEFAULT 2                   // BN254_OPT_KEY_DEDUP_FOLD: the keyed Miller loop of the dedup multiplies unit lines
#define KEY_DEDUP_MAX_KEYS_LIMIT 16384             // BN254_OPT_KEY_DEDUP_MAX_KEYS at most (338 MB of tables)
#define KD_MAX_PROBES 64u                          // open addressing: a longer probe sequence sends the call to the generic route
#define KD_EMPTY 0xFFFFFFFFu
enum { KD_OVERFLOW = 1, KD_DEGENERATE = 2 };
enum { KD_CTL_D = 0, KD_CTL_FLAGS, KD_CTL_KEYED_N, KD_CTL_GENERIC_N, KD_CTL_BUILD, KD_CTL_HITS, KD_CTL_DROPPED, KD_CTL_WORDS = 8 };
enum { KD_DROP_CAPACITY = 1, KD_DROP_RESET = 2 };  // KD_CTL_DROPPED: the call's misses did not fit the free rows / the host asked for an empty cache
struct KeyDedup {
  uint32_t* table;     // [slot_mask + 1] representative item of the slot, KD_EMPTY
  uint32_t* slot_id;   // [slot_mask + 1] key id of the slot (written by its representative)
  uint32_t* slot_of;   // [n] slot of the item (KD_EMPTY: probe overflow)
  uint32_t* key_idx;   // [n] key id of the item
  uint32_t* rep;       // [max_keys] representative item of the key
  uint32_t* ctl;       // [KD_CTL_WORDS] distinct keys D, flags, item counts of the keyed / generic Miller kernel
  int32_t* lines;      // [max_keys][87][c0, c1][re, im][9]
  int32_t* c2;         // [max_keys][KD_FOLD_KEY_WORDS] raw c2 of the lines of a key being built: [87][re, im][9] at the head of ...
  int32_t* fold;       // ... [max_keys][22][K0 .. K4][re, im][9] the folded rows (bn254_keydedup.h: kd_fold_pair), cached and dropped with `lines`.
                       // ONE buffer (fold == c2): a row's raw c2 is dead once k_kd_scale has loaded it into the leaves of its tree, and
                       // the workgroup that did so writes the row's folded rows over it at its end
  uint8_t* st;         // [max_keys] decode status of the representative
  uint8_t* inf;        // [max_keys] identity flag
  uint32_t* row_of;    // [max_keys] table row of the call's key id (k_kd_match)
  uint32_t* build_row; // [max_keys] rows of the keys this call builds, in the order of their ids: KD_CTL_BUILD entries
  uint32_t* build_rep; // [max_keys] ... and the item that represents each of them
  // the key cache (BN254_OPT_KEY_CACHE): the rows of lines / st / inf below c_state[0] persist between calls, found again by the key's bytes
  uint32_t* c_keys;    // [max_keys][32] the 128 bytes of the key of each row (the context's own copy)
  uint32_t* c_index;   // [index_mask + 1] open addressing over the rows' keys: row, KD_EMPTY
  uint32_t* c_state;   // [1] rows in use
  uint32_t slot_mask, hash_mask, max_keys, min_mult, index_mask;
};
// cache_reset: the cache is emptied before this call looks its keys up; cache_on = 0: ... and stays empty (every call builds all its keys)
__attribute__((visibility("hidden"))) int bn254_kd_enqueue(const uint8_t* d_pks, size_t n, uint32_t flags, KeyDedup kd, int force_generic, int cache_reset,
                                                           int cache_on, hipStream_t s);
// per-item and per-key bytes of the buffers above (slot arrays: at most 4n words each, the next power of two >= 2n)
#define KD_BYTES_PER_ITEM ((size_t)(2 * 4 + 2) * sizeof(uint32_t))
// (per key besides lines and folded rows / raw c2: rep, row_of, build_row, build_rep, the cache's copy of the key and four index slots, st, inf)
#define KD_FOLD_KEY_WORDS (BN_N_FOLD_ROWS * BN_KEY_FOLD_WORDS)
static_assert(KD_FOLD_KEY_WORDS >= BN_N_FIXED_LINES * 2 * BN_LIMBS, "a key's raw c2 fits where its folded rows go");
#define KD_BYTES_PER_KEY ((size_t)(BN_N_FIXED_LINES * BN_KEY_LINE_WORDS + KD_FOLD_KEY_WORDS) * sizeof(int32_t) + (4 + 32 + 4) * sizeof(uint32_t) + 2)

// entry points of bn254_trio.hip (octet layout for small batches)
__attribute__((visibility("hidden"))) int bn254_trio_miller_verify(size_t n, Ws ws, hipStream_t s, int mode = 0);
// entry points of bn254_quad.hip (the same with the four lane pairs of a verify as four waves with roles)
__attribute__((visibility("hidden"))) int bn254_quad_miller_verify(size_t n, Ws ws, hipStream_t s, int mode = 0);
__attribute__((visibility("hidden"))) int bn254_w8_miller_verify(size_t n, Ws ws, hipStream_t s, int mode = 0);      // eight waves per 32 verifies
// can the current device hold one workgroup of the small-batch kernels with the dynamic LDS they ask for (up to 156 KB)?
// Asked of the runtime's occupancy calculator at context creation; a runtime that cannot answer counts as "yes".
__attribute__((visibility("hidden"))) bool bn254_trio_fits_device();
__attribute__((visibility("hidden"))) bool bn254_quad_fits_device(int eight_waves);
__attribute__((visibility("hidden"))) int bn254_trio_final_exp(size_t n, Ws ws, int use_hash, uint8_t* status_out, hipStream_t s);
// entry points of bn254_lmiller.hip (Miller loop of the smallest batches as the lane machine: nine lane pairs in each of four waves per verify)
__attribute__((visibility("hidden"))) bool bn254_lm_fits_device();
__attribute__((visibility("hidden"))) int bn254_lm_miller_verify(size_t n, Ws ws, hipStream_t s, int mode = 0);
__attribute__((visibility("hidden"))) int bn254_lm_g2_subgroup(size_t n, Ws ws, hipStream_t s, int fail_status = 4 /* ST_INVALID_GROUP_POINT; the compressed decoders report ST_NOT_MEMBER */);   // the G2 subgroup test of points already decoded into the Q planes
// entry points of bn254_nonet.hip (final exponentiation of the smallest batches on nine lane pairs per verify)
__attribute__((visibility("hidden"))) bool bn254_nonet_fits_device();
__attribute__((visibility("hidden"))) int bn254_nonet_final_exp(size_t n, Ws ws, int use_hash, uint8_t* status_out, hipStream_t s, int wide = 0);
__attribute__((visibility("hidden"))) int bn254_nonet_final_exp_product(size_t n, size_t k, Ws ws, uint8_t* gt_out, uint8_t* status_out, hipStream_t s);   // bn254_batch_pairing*, n <= NONET_WIDE_MAX_BATCH
#endif  // BN_WS_ROUTE_ONLY
