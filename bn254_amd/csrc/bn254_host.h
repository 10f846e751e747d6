// Host side shared by the translation units that implement the C ABI (include/bn254_hip.h): the context, its buffers, and the launchers of
// the kernels more than one unit needs.  bn254_hip.hip owns the definitions; everything here is internal to libbn254hip.so (hidden).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/bn254_hip.h"

#define BN_HIDDEN __attribute__((visibility("hidden")))

// aggregate verify: which of the context's pool buffers hold valid tables, and for which pools (bn254_group.hip: agg_build_tables)
// t4_builder: how the 4-signer signature tables were built — 0 not at all, 1 pairs + quads (the pair table is in pool[7]), 2 k_pool_subsets_g1
struct AggTables { int valid; size_t n_msgs, n_signers, n_groups, groups4, built_for; int wide2, wide1, t4_builder; };

// where a randomised call over groups left them for its debug hook: S_g in the P1 planes from cbase, the table pairs from tbase, the rest in
// the call's scratch buffer
struct AggrLast { size_t ng, cbase, tbase; const uint32_t *nagg, *bkey; const uint64_t *glo, *ghi; const uint8_t* gst; };

// the order in which a profiled call recorded its events: decode, hash, Miller loop, final exponentiation between ev[0] .. ev[4]; the
// host-pointer verify's hash, decode, ...; or the collect call's (its select-and-sum runs last and reports in ms[1]): front end ev[1]..ev[2],
// Miller loop ..ev[3], final exponentiation ..ev[4], select-and-sum ..ev[0]
// (the optimistic collect records its four intervals in order: EV_DECODE_FIRST)
enum EvLayout { EV_DECODE_FIRST = 0, EV_HASH_FIRST = 1, EV_COLLECT = 2 };

struct bn254_ctx {
  int device;
  hipStream_t stream;
  Ws ws;
  // staging buffers for the host-pointer entry points (device memory, grown on demand)
  uint8_t* stage[8];
  size_t stage_cap[8];
  int profiling;
  int split_miller;  // A/B knob: one pairing per lane (k_miller_verify_split) instead of the fused 2-pair loop
  Pool pool[8];       // aggregate verify: pk pool, sig pool, H(m) pool, subset sums of the pk pool and of the signature pool, and their widened
                      // forms (16 keys / 8 signatures per entry) for the largest batches (grown on demand)
  size_t pool_fp[8];  // coordinates per entry: 4, 2, 2, 4, 2, 4, 2, 2 ([7]: the pair table the 4-signer signature tables are built from)
  int agg_wide_min_tuples;    // aggregate verify: the widened tables from this many tuples on (0 = never)
  int agg_subset_min_tuples;  // aggregate verify: tabulate subset sums of the pk pool for batches of at least this many tuples (0 = never)
  int agg_sort_by_msg;        // aggregate verify: bucket the tuples by message before the aggregation kernel (default 1; A/B and test knob)
  int agg_t4_route;           // BN254_OPT_AGG_T4_ROUTE (developer option): 0 = the 4-signer signature tables from pairs + quads, 1 = from k_pool_subsets_g1
  int pair_lanes;    // verify: Miller loop + final exponentiation on lane pairs (bn254_pair.hip); default on
  int rand_min_batch;      // randomised verify: batches below this size run the exact kernels (default RAND_MIN_BATCH_DEFAULT)
  int rand_items_per_lane; // randomised verify: 0 = by batch size, 1 or 2 forced (A/B and tests)
  int hash_max_tries; // test knob: counters tried before HashToPointError (0 = the reference's 255)
  int trio_wave_roles; // octet layout: the Miller loop's four lane pairs as the four waves of a workgroup (k_miller_verify_quad) instead of one wave
  int hash_direct_width; // small batches: counters tried at once with the square root itself (k_hash_direct); 0 = rounds only
  int hash_schedule;     // BN254_OPT_HASH_SCHEDULE: 0 = by size, 1 = always the multi-round schedule, 2 = the wide round and tail above HASH_DIRECT_MAX_N
  int hash_wide_width;   // BN254_OPT_HASH_WIDE_WIDTH (measurement knob): counters per message in the wide schedule's round; 0 = by size
  int hash_tail_chunk;   // BN254_OPT_HASH_TAIL_CHUNK (test seam): counters a survivor's lane group tries at once in the tail (default 32)
  int trio_max_batch; // verify / check_public_keys batches up to this size run in the octet layout (bn254_trio.hip); 0 = never
  int lm_max_batch;    // ... and up to this size their Miller loop runs as the lane machine (bn254_lmiller.hip); 0 = never
  int nonet_wide;      // ... on eighteen lane pairs (one verify per wave) while the batch is at most one verify per SIMD (BN254_OPT_NONET_WIDE)
  int nonet_max_batch; // ... and up to this size their final exponentiation runs on nine lane pairs per verify (bn254_nonet.hip); 0 = never
  hipEvent_t ev[5];
  int ev_valid;
  int ev_layout;       // EvLayout: which intervals the five events of the last profiled call bracket (bn254_ctx_last_kernel_ms); set with ev_valid, by prof_done
  hipStream_t copy_stream;   // host-pointer verify: signatures and keys cross PCIe here while the hash rounds run on `stream`
  uint8_t* pin;              // ... through this PINNED host buffer (hipHostMalloc, grown on demand): BN254_OPT_PINNED_STAGING
  size_t pin_cap;
  int pinned_staging;        // 0 = hipMemcpyAsync straight from the caller's (pageable) buffers
  hipEvent_t copy_done;
  uint64_t msgs_len_next;    // bn254_ctx_expect_msgs_len: size of the d_msgs buffer of the NEXT call that hashes messages
  int msgs_len_declared;
  uint64_t msgs_len_call;    // ... as taken by the entry point now running (MsgsLenScope); UINT64_MAX = not declared
  int entry_depth;           // the host-pointer entry points call their *_device forms: only the outermost one takes the declaration
  int32_t* key_lines;        // keyed verify: registered keys (bn254_ctx_register_keys), see KeyTable in bn254_ws.h
  int32_t* key_xy;           // ... and their affine coordinates (4 x 9 words per key) for the small-batch route
  uint8_t* key_st;
  uint8_t* key_inf;
  size_t n_keys, key_cap;
  hipEvent_t last_done;      // recorded on the CALLER's stream when a *_device call on such a stream returns (CallDone below): what ctx_quiesce
  bool last_done_armed;      // waits for.  The context keeps no handle of a stream it does not own — the caller may destroy its stream any time.
  Pool g2_comb;              // fixed-base table of the G2 generator for key derivation (bn254_group.hip: g2_comb_build), built at the first keygen call
  int g2_comb_ready;
  Pool g1_comb;              // ... and of the G1 generator (PublicKeyG1::from_private_key)
  int g1_comb_ready;
  int g2_fixed_base;         // BN254_OPT_G2_FIXED_BASE (developer option, default 1): key derivation through the comb table; 0 = the 256-step ladder
  AggTables reg_pools;       // bn254_ctx_register_pools: the tables of the registered pools (valid until the next registration or raw-pool call)
  int max_chunk;             // BN254_OPT_MAX_CHUNK: verify-shaped batches above this size are processed in slices (0 = only when the workspace would not fit)
  int assume_free_mb;        // test knob (BN254_OPT_ASSUME_FREE_MB): the automatic rule prices the workspace against this much free memory instead of hipMemGetInfo
  bool fits_w8, fits_quad, fits_trio;   // the device can hold a workgroup of the small-batch kernels (LDS), asked at creation
  uint8_t* aggd_buf;         // aggregate verify over distinct messages: the per-aggregate scans, the slot map and the partials' ids (bn254_aggd_plan.h: AggdScratch)
  size_t aggd_cap;
  int key_dedup;             // BN254_OPT_KEY_DEDUP: verify on lane pairs finds the batch's distinct keys and runs the keyed Miller loop (bn254_keydedup.hip)
  int kd_max_keys;           // BN254_OPT_KEY_DEDUP_MAX_KEYS
  int kd_min_mult;           // BN254_OPT_KEY_DEDUP_MIN_MULT
  int kd_force_generic;      // BN254_OPT_KEY_DEDUP_FORCE_GENERIC (developer hook): 1 = the device-side decision always says "generic", 2 = the builder reports a degenerate line
  int kd_fold;               // BN254_OPT_KEY_DEDUP_FOLD (developer option): 1 = the keyed Miller kernel on the folded rows (k_miller_verify_keyed_fold_pair), 2 = on unit lines (k_miller_verify_keyed_unit_pair), 0 = line pairs
  int kd_hash_bits;          // BN254_OPT_KEY_DEDUP_HASH_BITS (test seam): bits of the key hash kept (0 = all), to force collisions
  hipStream_t kd_stream;     // the dedup and the table builder run here, forked from and joined into the call's stream
  hipEvent_t kd_fork, kd_join;
  hipEvent_t kd_done;        // recorded behind a dedup call on ITS stream; the next dedup call waits for it on the device before it touches the dedup buffers
  int kd_cache;              // BN254_OPT_KEY_CACHE: the line tables stay between calls, a call builds only the keys it has not seen (default 1)
  bool kd_cache_valid;       // ... the device-side cache holds what the last dedup call left (false: the next call empties it first)
  uint32_t kd_cache_flags;   // ... and what its rows were built under: decode flags, KEY_DEDUP_MAX_KEYS, KEY_DEDUP_HASH_BITS
  int kd_cache_max_keys, kd_cache_hash_bits;
  uint8_t* kd_buf;           // KeyDedup buffers (bn254_ws.h), grown on demand
  size_t kd_items_cap, kd_keys_cap;
  uint32_t* kd_ctl;          // the device-side decision of the last call that ran the dedup (bn254_debug_key_dedup_last)
  const int32_t* kd_lines_last;   // ... and its tables, representatives, statuses and identity flags (bn254_debug_key_tables; into kd_buf)
  const int32_t* kd_fold_last;    // ... its folded rows (bn254_debug_key_fold_tables)
  const uint32_t* kd_rep_last;
  const uint32_t* kd_row_of_last;   // ... key id of that call -> row of the tables
  const uint8_t *kd_st_last, *kd_inf_last;
  int kd_last_run;           // ... and whether the last bn254_batch_verify_device ran it at all
  int aggd_keyed_route;      // BN254_OPT_AGGD_KEYED_ROUTE (test and measurement knob): 0 by size, 1 / 2 the slot kernel of that width, 3 expanded keys
  int agg_rand_min_pairs;    // BN254_OPT_AGG_RAND_MIN_PAIRS: the randomised keyed aggregate verify from this many messages on
  int agg_rand_group_pairs;  // BN254_OPT_AGG_RAND_GROUP_PAIRS: messages per group of its combined checks (at least the number of keys)
  uint8_t* aggr_buf;         // ... its scratch (bn254_aggd_plan.h: AggrScratch), grown on demand
  size_t aggr_cap;
  uint32_t* aggr_stats;      // ... what its last run did on the device (bn254_debug_agg_rand_last)
  int aggr_last_ran;         // ... and whether the last call took the randomised route at all
  // ... and where that call left its groups (bn254_debug_agg_rand_sums): S_g in the P1 planes from cbase, the table pairs from tbase, the rest in aggr_buf
  AggrLast aggr_last;
  // signer bitmaps over the registered keys (bn254_bitmap.hip): the bad-bit vector and the subset tables of the set, built by the first
  // bitmap call after a registration (bn254_ctx_register_keys clears the two flags), grown on demand
  uint8_t* bm_bad;           // uint32 words, one bit per key
  size_t bm_bad_cap;
  uint8_t* bm_tab;           // records (160 B per entry), then the identity flags (1 B per entry)
  size_t bm_tab_cap;
  bool bm_bad_valid, bm_tab_valid;
  int bm_table_max_keys;     // BN254_OPT_BITMAP_TABLE_MAX_KEYS: tables while n_keys <= this (0 = never)
  int bm_route;              // BN254_OPT_BITMAP_ROUTE (developer option): 0 by the rule above, 1 always tables, 2 never
  // ... the voting weights of the registered keys (bn254_bitmap_out.hip: bn254_ctx_set_key_weights): byte-indexed tables of u64 subset sums,
  // 2 KB per 8 keys, grown on demand; a registration forgets them (register_keys_begin)
  uint8_t* bw_tab;
  size_t bw_tab_cap;
  bool bw_set;
  // ... randomised (bn254_bitmap_rand.hip), as the aggr_* members above
  int bmr_min_tuples;        // BN254_OPT_BITMAP_RAND_MIN_TUPLES: the randomised bitmap call from this many tuples on
  int bmr_group_tuples;      // BN254_OPT_BITMAP_RAND_GROUP_TUPLES: tuples per group of its combined checks
  int bmr_max_keys;          // BN254_OPT_BITMAP_RAND_MAX_KEYS: ... and only while the registered set has at most this many keys
  uint8_t* bmr_buf;          // its scratch, grown on demand
  size_t bmr_cap;
  uint32_t* bmr_stats;       // what its last run did on the device (bn254_debug_bitmap_rand_last); inside bmr_buf
  int bmr_last_ran;          // ... and whether the last call took the randomised route at all
  AggrLast bmr_last;         // ... and where it left its groups (bn254_debug_bitmap_rand_sums)
  // building signer-bitmap aggregates from shares (bn254_collect.hip)
  uint8_t* collect_buf;      // per tuple: H(m), its flags and the scans of the share ranges (ClScratch), grown on demand
  size_t collect_cap;
  int collect_wave_min;      // BN254_OPT_COLLECT_WAVE_MIN_SHARES: tuples with at least this many shares are summed by a wave each
  int collect_rand_min_shares;    // BN254_OPT_COLLECT_RAND_MIN_SHARES: the randomised collect from this many shares on
  int collect_rand_min_per_key;   // BN254_OPT_COLLECT_RAND_MIN_PER_KEY: ... and from this many shares per registered key on
  uint32_t* clr_stats;       // what the slices of its last call did on the device (bn254_debug_collect_rand_last); inside collect_buf
  int clr_last_ran;          // ... and whether that call took the randomised route at all
  int collect_opt_min_shares;       // BN254_OPT_COLLECT_OPT_MIN_SHARES: the optimistic collect from this many shares on
  int collect_opt_min_tuple_shares; // BN254_OPT_COLLECT_OPT_MIN_TUPLE_SHARES: ... and, per tuple, from this many candidates on
  uint32_t* clo_stats;       // what its last call did on the device (bn254_debug_collect_opt_last); inside collect_buf
  int clo_last_ran;          // ... and whether that call took the optimistic route at all
  int merge_wave_min;        // BN254_OPT_MERGE_WAVE_MIN_PARTS (bn254_merge.hip): tuples with at least this many partials are merged by a wave each
  int merge_opt_min_parts;   // BN254_OPT_MERGE_OPT_MIN_PARTS: the optimistic merge from this many partials on
  uint32_t* mgo_stats;       // what its last call did on the device (bn254_debug_merge_opt_last); inside collect_buf
  int mgo_last_ran;          // ... and whether that call took the optimistic route at all
  // proofs of possession (bn254_pop.hip): the composed messages TAG || pk, their offsets, and the second status array of a fold, grown on demand
  uint8_t* pop_buf;
  size_t pop_cap;
  // threshold signatures and the scalar-weighted sum (bn254_threshold.hip): a Jacobian term and its status per share / term, and for the
  // threshold call the coefficients, the take flags and the second claim rows, grown on demand
  uint8_t* th_buf;
  size_t th_cap;
  // ... the optimistic threshold call: the GROUP key (bn254_ctx_set_group_key) in a one-entry key table of its own — lines, status byte,
  // identity byte, affine words, as k_register_keys leaves one key — allocated by the first call that sets one; a registration forgets it
  int32_t *gk_lines, *gk_xy;
  uint8_t *gk_st, *gk_inf;
  bool gk_set;
  int pe_wave_min;           // BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS (bn254_polyeval.hip): polynomials with at least this many coefficients are evaluated by a wave each
  int th_opt_min_shares;     // BN254_OPT_THRESHOLD_OPT_MIN_SHARES: the optimistic threshold call from this many shares on
  uint32_t* tho_stats;       // what its last call did on the device (bn254_debug_threshold_opt_last); inside collect_buf
  int tho_last_ran;          // ... and whether that call took the optimistic route at all
  // compressed G1 input of the registered-key calls (bn254_g1stage.hip): per item the 64 bytes the call reads in its place, then the pre-status
  // bytes, grown on demand
  uint8_t* g1c_buf;
  size_t g1c_cap;
};

struct ScopedEvents {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t create() {
    hipError_t e = hipEventCreate(&e0);
    return e == hipSuccess ? hipEventCreate(&e1) : e;
  }
  ~ScopedEvents() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  ScopedEvents() = default;
  ScopedEvents(const ScopedEvents&) = delete;
  ScopedEvents& operator=(const ScopedEvents&) = delete;
};
// the context's thresholds as the routing table's limits (bn254_ws.h: bn_route) — every size-dependent choice of layout goes through here
static inline BnRouteLimits route_limits(const bn254_ctx* c) {
  BnRouteLimits L;
  L.small_max = c->pair_lanes && c->trio_max_batch > 0 ? (size_t)c->trio_max_batch : 0;
  L.lm_max = c->lm_max_batch > 0 ? (size_t)c->lm_max_batch : 0;
  L.nonet_max = c->nonet_max_batch > 0 ? (size_t)c->nonet_max_batch : 0;
  L.nonet_wide_max = c->nonet_wide ? (size_t)NONET_WIDE_MAX_BATCH : 0;
  return L;
}
static inline BnRoute route_for(const bn254_ctx* c, size_t n) { return bn_route(route_limits(c), n); }
// the decode-time helpers of the smallest batches (G2 subgroup ladder on the lane machine's level tables; the pairing API's small-batch
// kernels) follow the lane machine's own threshold, whatever the size of the small-batch family
static inline bool route_lane_machine_helpers(const bn254_ctx* c, size_t n) { return c->pair_lanes && c->lm_max_batch > 0 && n <= (size_t)c->lm_max_batch; }
static inline unsigned grid_for(size_t n) { return (unsigned)((n + BN_WAVE - 1) / BN_WAVE); }

// before a buffer of the context is freed or rewritten: wait for the context's own streams and for the END of its last *_device call on a
// caller's stream (an event the context owns) — not for the whole device (other contexts, other streams and a stream capture running
// elsewhere in the process are left alone)
BN_HIDDEN int ctx_quiesce(bn254_ctx* c);
// Opened by every *_device entry point once it knows its stream: on every exit path (errors included — kernels may have been enqueued)
// the context's own event is recorded behind whatever the call put on a caller's stream.  Nothing is recorded for the context's own stream
// (ctx_quiesce synchronises that one directly), so the default path pays nothing.
struct CallDone {
  bn254_ctx* c;
  hipStream_t s;
  CallDone(bn254_ctx* ctx, hipStream_t stream) : c(ctx), s(stream) {}
  ~CallDone() {
    if (s == c->stream) return;
    if (hipEventRecord(c->last_done, s) == hipSuccess) c->last_done_armed = true;
    else (void)hipGetLastError();                    // e.g. a stream under capture: nothing of this call can outlive the capture's owner
  }
  CallDone(const CallDone&) = delete;
  CallDone& operator=(const CallDone&) = delete;
};
BN_HIDDEN int ws_reserve(bn254_ctx* c, size_t n);
// Oversized batches: the slice length the verify-shaped entry points cut a batch of n items into, or 0 = one piece.  BN254_OPT_MAX_CHUNK when
// set; otherwise only when the workspace of the whole batch (WS_BYTES_PER_ITEM each) would not fit what the device has free (+ what the
// context's present workspace would give back): then the largest multiple of 65 536 items that fits in 80 % of it.
// ws_per_item: workspace entries per item (2 with BN254_OPT_SPLIT_MILLER); key_dedup: the call also reserves the key-dedup buffers (bn254_ws.h:
// KD_BYTES_PER_ITEM per item + KD_BYTES_PER_KEY per key of BN254_OPT_KEY_DEDUP_MAX_KEYS)
BN_HIDDEN size_t ws_chunk_for(bn254_ctx* c, size_t n, size_t ws_per_item = 1, bool key_dedup = false);
// An oversized *_device verify: slice(lo, len) sends items [lo, lo + len) through the same entry point, one slice after the other on the
// caller's stream — the offsets are absolute into d_msgs, so a slice is the same arrays further in; statuses land at the items' own positions
// (profiling: the last slice's).  The host-pointer forms slice in bn254_hip.hip: verify_host_sliced.
template <class Slice> static inline int verify_device_sliced(size_t n, size_t chunk, Slice slice) {
  for (size_t lo = 0; lo < n; lo += chunk)
    if (const int rc = slice(lo, n - lo < chunk ? n - lo : chunk)) return rc;
  return 0;
}
// a device buffer of the context grown on demand to at least `bytes` (quiesce, free, allocate a multiple of 4 096): the staging slots,
// and the scratch of the aggregate calls over distinct messages (aggd_buf, aggr_buf)
BN_HIDDEN int scratch_reserve(bn254_ctx* c, uint8_t** buf, size_t* cap, size_t bytes);
BN_HIDDEN int stage_reserve(bn254_ctx* c, int slot, size_t bytes);
BN_HIDDEN int pool_reserve(bn254_ctx* c, int which, size_t n_fp, size_t entries);
BN_HIDDEN int pool_reserve_one(bn254_ctx* c, Pool* p, size_t n_fp, size_t entries);
static inline bool misaligned(const void* p) { return ((uintptr_t)p & 3u) != 0; }
// host-pointer entry points: an offsets array (n + 1 entries) must be non-decreasing — a kernel computes lengths as
// off[i+1] - off[i], and a wrapped length walks far outside the staged buffer.  O(n) on memory the host already has.
// (The *_device variants cannot look: there the kernels check every span themselves, include/bn254_hip.h.)
static inline bool offsets_ok(const uint64_t* off, size_t n) {
  for (size_t i = 0; i < n; ++i) if (off[i] > off[i + 1]) return false;
  return true;
}
// ... and the messages those offsets index: bytes to stage (off[n] > 0) need a buffer to stage them from
static inline bool msgs_ok(const uint8_t* msgs, const uint64_t* off, size_t n) { return offsets_ok(off, n) && (off[n] == 0 || msgs); }
// bn254_ctx_expect_msgs_len is consumed by the NEXT entry point that hashes messages — whatever that call goes on to do: every such
// entry point opens with a MsgsLenScope, which takes the declaration and clears it before any argument check, staging step or
// allocation can return early (a declaration left armed would bound-check an unrelated later call against the wrong length).
struct MsgsLenScope {
  bn254_ctx* c;
  explicit MsgsLenScope(bn254_ctx* ctx) : c(ctx) {
    if (c && c->entry_depth++ == 0) {
      c->msgs_len_call = c->msgs_len_declared ? c->msgs_len_next : UINT64_MAX;
      c->msgs_len_declared = 0;
    }
  }
  ~MsgsLenScope() { if (c) --c->entry_depth; }
  MsgsLenScope(const MsgsLenScope&) = delete;
  MsgsLenScope& operator=(const MsgsLenScope&) = delete;
};
// The staging of a host-pointer entry point: the caller's buffers cross into the context's numbered slots (c->stage[slot]) on c->stream,
// the outputs come back the same way.  Those copies read and write the caller's memory until the streams drain, so a HostStaging keeps
// one rule on every path out: a call that has opened one returns only after c->stream and c->copy_stream are idle — finish() on the way
// out, the destructor on an early return.  Errors are sticky: after the first one in() / out() do nothing, no copy goes back, and
// finish() returns it.  The caller numbers the slots, because calls nest: mul_host -> *_mul_device -> comb_build stages into 5 .. 7
// while mul_host holds 0 .. 3.
struct BN_HIDDEN HostStaging {
  bn254_ctx* c;
  int rc = 0;                                              // the call's first error
  explicit HostStaging(bn254_ctx* ctx) : c(ctx) {}
  ~HostStaging() { if (!finished) (void)drain(); }
  bool ok() const { return rc == 0; }
  void check(hipError_t e) { if (!rc && e != hipSuccess) rc = -(int)e; }
  uint8_t* in(int slot, const void* host, size_t bytes);   // reserve the slot and enqueue the H2D copy: the slot's device pointer
  uint8_t* out(int slot, size_t bytes, void* host = nullptr);   // reserve the slot: its device pointer; finish() copies it to `host`
  void copy_back(void* host, const void* dev, size_t bytes);      // ... the same for device memory outside the slots
  int finish();      // unless the call has failed, enqueue the copies back; wait: the call's first error, else the wait's
  HostStaging(const HostStaging&) = delete;
  HostStaging& operator=(const HostStaging&) = delete;
 private:
  hipError_t drain();                                      // wait for c->stream and c->copy_stream
  struct Back { void* host; const void* dev; size_t bytes; } back[6];
  int n_back = 0;
  bool finished = false;
};

// Enqueue the hash-to-G1 rounds for n messages; points land in planes (px, px+1), statuses in BY_ST_HASH.

// the end of every profiled call: the events are valid and this is their order — one assignment, so a call cannot leave the other's layout behind
static inline void prof_done(bn254_ctx* c, int layout) { if (c->profiling) { c->ev_valid = 1; c->ev_layout = layout; } }
#define PROF_MARK(idx) do { if (c->profiling) HIP_TRY(hipEventRecord(c->ev[idx], s)); } while (0)

// launchers of kernels that live in bn254_hip.hip and are used by other units too (a kernel is launched from the unit that defines it)
BN_HIDDEN int launch_decode_g1(bn254_ctx* c, hipStream_t s, const uint8_t* d_pts, size_t n, uint32_t flags, int px, int inf_plane, int accumulate);
BN_HIDDEN int launch_decode_g2(bn254_ctx* c, hipStream_t s, const uint8_t* d_pts, size_t n, uint32_t flags, int accumulate);
BN_HIDDEN int launch_hash_rounds(bn254_ctx* c, hipStream_t s, const uint8_t* d_msgs, const uint64_t* d_off, size_t n, int px, int inf_plane,
                                 uint8_t* d_tries, int mark_finish = -1);
// the final exponentiation of a verify-shaped batch in the layout `fe` (BnFeLayout) of its routing-table row
BN_HIDDEN int launch_final_exp_layout(bn254_ctx* c, hipStream_t s, size_t n, int use_hash, uint8_t* d_status, int fe);
// what the Miller loop of a verify-shaped batch computes (the `mode` of the Miller kernels): a verify's miller(H(m), pk) * miller(sig, -G2), or
// check_public_keys' miller(G1::one(), pk_g2) * miller(pk_g1, -G2)
enum BnVerifyPairs { BN_PAIRS_VERIFY = 0, BN_PAIRS_CHECK_PKS = 1 };
// the Miller loop and final exponentiation of such a batch whose planes are filled, in the layouts BN254_OPT_PAIR_LANES, _TRIO_WAVE_ROLES and
// the routing table choose; mark: profiling event 3 between the two
BN_HIDDEN int launch_verify_miller_fe(bn254_ctx* c, hipStream_t s, size_t n, int pairs, int use_hash, uint8_t* d_status, bool mark);
// the same for a KEYED batch (bn254_rand.hip): item i's key is the registered key d_key_idx[i] — rule 2 of bn254_batch_verify_keyed behind the
// decode status, then the routing table's keyed kernels; and the statuses of such a batch when no key is registered
// kt, key_xy: the table the indices point into — the context's registered set (ctx_key_table), or the group key's one entry
BN_HIDDEN int launch_keyed_miller_fe(bn254_ctx* c, hipStream_t s, size_t n, const uint32_t* d_key_idx, uint8_t* d_status, const KeyTable& kt,
                                     const int32_t* key_xy);
static inline KeyTable ctx_key_table(const bn254_ctx* c) { const KeyTable kt = {c->key_lines, c->key_st, c->key_inf, (uint32_t)c->n_keys}; return kt; }
BN_HIDDEN int launch_keyed_no_keys(bn254_ctx* c, hipStream_t s, size_t n, uint8_t* d_status);
// a registration in two steps (bn254_rand.hip), shared by bn254_ctx_register_keys and bn254_ctx_register_keys_pop: quiesce, drop the previous set
// (n_keys = 0, the bitmap call's vector and tables invalid) and make room for n_keys keys; then decode and tabulate the staged keys on c->stream.
// The caller sets c->n_keys once the new set stands.
BN_HIDDEN int register_keys_begin(bn254_ctx* c, size_t n_keys);
BN_HIDDEN int launch_register_keys(bn254_ctx* c, const uint8_t* d_pks, size_t n_keys, uint32_t flags);
// ... and its RANDOMISED form (bn254_rand.hip; the body of bn254_batch_verify_keyed_randomized behind decode and hash): the items that pass
// rules 1-3 grouped by key in runs of 64, every group one combined check, the items of a failing group re-checked exactly through the
// workspace's h_list / h_cnt queue.  Item i's weight is rand_scalar(seed, index_base + i).  mode: 0 = 128-bit weights, 1 = 64-bit, 2 = GLV.
// Records profiling event 3 between the scalar ladders and the group checks.  The caller reserves, BEFORE its first kernel, what
// keyed_rand_need names (keyed_rand_reserve does); the launcher refuses a call that did not.
struct RandSeed { uint32_t w[8]; };
static inline RandSeed rand_seed_from(const uint8_t* seed32) {
  RandSeed seed;
  for (int j = 0; j < 8; ++j)
    seed.w[j] = ((uint32_t)seed32[4 * j] << 24) | ((uint32_t)seed32[4 * j + 1] << 16) | ((uint32_t)seed32[4 * j + 2] << 8) | seed32[4 * j + 3];
  return seed;
}
static inline int rand_mode_of(uint32_t flags) { return (flags & BN254_FLAG_RAND64) ? 1 : (flags & BN254_FLAG_RAND_GLV) ? 2 : 0; }
// n items over the registered set: the group slots start at workspace entry gbase, behind the items; at most groups_max groups (every key's
// run is padded to whole groups of 64); ws_entries workspace entries, `words` uint32 of stage slot 5, groups_max bytes of stage slot 7
struct KeyedRandNeed { size_t gbase, groups_max, ws_entries, words; };
static inline KeyedRandNeed keyed_rand_need(const bn254_ctx* c, size_t n) {
  KeyedRandNeed r;
  const size_t K = c->n_keys;
  r.groups_max = n / BN_WAVE + (K < n ? K : n) + 1;
  r.gbase = (n + 255) & ~(size_t)255;
  r.ws_entries = r.gbase + r.groups_max;
  r.words = 2 * K + 2 + r.groups_max + r.groups_max * BN_WAVE;
  return r;
}
static inline int keyed_rand_reserve(bn254_ctx* c, size_t n) {
  const KeyedRandNeed need = keyed_rand_need(c, n);
  int rc = ws_reserve(c, need.ws_entries);
  if (!rc) rc = stage_reserve(c, 5, need.words * sizeof(uint32_t));
  if (!rc) rc = stage_reserve(c, 7, need.groups_max);
  return rc;
}
// where the last launch left {groups, slots in use} and the groups' verdicts (0 = passed)
static inline uint32_t* keyed_rand_meta(const bn254_ctx* c) { return (uint32_t*)c->stage[5] + 2 * c->n_keys; }
static inline uint8_t* keyed_rand_group_st(const bn254_ctx* c) { return c->stage[7]; }
BN_HIDDEN int launch_keyed_rand_checks(bn254_ctx* c, hipStream_t s, size_t n, const uint32_t* d_key_idx, const RandSeed& seed, int mode,
                                       uint64_t index_base, uint8_t* d_status);
// one lane per item: k_miller_verify (map / count: a device-side queue of items, or null) and k_final_exp (the arguments of the kernel)
// one lane per pairing: k_miller_var (f = miller(P1, Q) at every index below n), k_rand_tail (bn254_rand.hip: F_g * miller(S_g, -G2) at gbase + g)
BN_HIDDEN int launch_miller_var_lane(bn254_ctx* c, hipStream_t s, size_t n);
BN_HIDDEN int launch_rand_tail_lane(bn254_ctx* c, hipStream_t s, size_t n_groups, size_t gbase);
BN_HIDDEN int launch_miller_verify_lane(bn254_ctx* c, hipStream_t s, size_t n, const uint32_t* map, const uint32_t* count);
BN_HIDDEN int launch_final_exp_lane(bn254_ctx* c, hipStream_t s, size_t n, size_t k, size_t item_stride, size_t pair_stride, int use_hash, uint8_t* gt_out,
                                    uint8_t* status_out, int raw_only, size_t base, const uint32_t* map, const uint32_t* count);
// signer bitmaps (bn254_bitmap.hip): does a call read the subset tables; the bad-bit vector and, when read, the tables built on the call's stream
BN_HIDDEN bool bm_wants_tables(const bn254_ctx* c);
BN_HIDDEN int bm_prepare(bn254_ctx* c, hipStream_t s, bool tables);
// ... and the aggregate keys of n tuples (row i of d_bits -> the Q planes of workspace entry i, rule 2 behind the entry's decode status)
BN_HIDDEN int launch_bitmap_sum(bn254_ctx* c, hipStream_t s, const uint32_t* d_bits, size_t bm_words, size_t n, bool tables);
// the collect family (bn254_collect.hip), shared with the merge of partial aggregates (bn254_merge.hip).  Per tuple, outside the (sliced)
// workspace: the scans of the range rule, H(m) with its identity flag and hash status; in front the counters of the randomised and the
// optimistic collect, behind the optimistic route's flag and verdict
struct ClScratch { uint32_t* stats; uint64_t *mx, *hi, *end, *tot; int32_t* hpt; uint8_t *hinf, *hst, *flag, *verdict; };
// stats: {slices, groups checked, groups failed, shares re-checked exactly} of the randomised collect, then from CLO_STAT_AT what an optimistic
// route did — the collect's or the merge's, whichever call owns the scratch: {tuples checked, passed, sent the exact way, items verified exactly}
#define CL_STAT_WORDS 8
#define CLO_STAT_AT 4
// ... carved for n tuples from the context's collect_buf (grown on demand: before the call's first kernel)
BN_HIDDEN int cl_scratch_reserve(bn254_ctx* c, size_t n, ClScratch* S);
// The arguments of one call of the family, built once by its extern "C" function: n tuples of a message and a range of ITEMS (64 bytes each
// — the collect's and the threshold call's shares, the merge's partials), item j with aux[j] (the collect: its key index; the merge: its
// bitmap row, bm_words words).  A host form holds the caller's pointers, its device form the staged ones (cl_stage).
struct ClCall {
  const uint8_t* msgs;
  const uint64_t* msg_off;                             // n + 1
  const uint8_t* items;
  const uint32_t* aux;
  const uint64_t* off;                                 // n + 1, into the items
  size_t n_items, n, bm_words;
  uint32_t flags;
  uint8_t *item_status, *item_taken;                   // per item; taken: the merge only, else null
  uint8_t *tuple_status, *agg_sigs;                    // per tuple: 1 and 64 bytes
  uint32_t *signer_bits, *n_signers;                   // per tuple: bm_words words, and the count (or null)
};
// the collect's and the threshold call's own check (ahead of the common ones: n == 0 does not excuse it): a bitmap that cannot hold a
// registered key cannot describe the result; and the items' keys
static inline bool cl_keys_ok(const bn254_ctx* c, const ClCall& a) { return c && a.bm_words >= (c->n_keys + 31) / 32 && !(a.n && a.n_items && !a.aux); }
// What every form checks: the context, the 32-bit bounds, the null pointers; n == 0 returns 0; then a host form selects the device and reads
// the offsets it was given (msgs_ok, and a.off from 0 to n_items without a step back), a device form looks at the alignment and selects
// the device.  false = the call returns *rc now.
BN_HIDDEN bool cl_checks_host(bn254_ctx* c, const ClCall& a, int* rc);
BN_HIDDEN bool cl_checks_device(bn254_ctx* c, const ClCall& a, int* rc);
// The staging of a host form: the inputs into slots 0 .. 4 (aux_words: uint32 per item of a.aux), every output into slot out_slot — the
// aligned ones first — with its copy home registered; *d = the same call on the staged buffers.
BN_HIDDEN void cl_stage(HostStaging& st, const ClCall& a, size_t aux_words, int out_slot, ClCall* d);
// ... the hash of the n messages, once per tuple in pieces of t_piece, and the range rule over the n + 1 offsets a.off into n_items items:
// a.tuple_status, and S.end for the item -> tuple search
BN_HIDDEN int cl_hash_and_plan(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t t_piece, const ClScratch& S);
// ... and the head of a slice of items lo .. lo + len: their decode into workspace entries 0 .. len and, beside each, H(m) and the hash
// status of its tuple (an item of no accepted tuple: the generator, decode status 2).  A slice behind the first opens its own front end.
BN_HIDDEN int cl_slice_head(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t lo, size_t len, const ClScratch& S);
// The exact collect behind the checks of its entry point (seed32: the randomised one; optimistic), for the threshold call as for the
// collect's own: every buffer reserved, then the whole call enqueued on s.  *S = the scratch it carved, for what the caller enqueues behind.
BN_HIDDEN int cl_collect_run(bn254_ctx* c, const ClCall& call, const uint8_t* seed32, bool optimistic, hipStream_t s, ClScratch* S);
// The two stages the optimistic collect and the optimistic merge share.  The tuple check: in pieces of t_piece tuples
// the call's own aggregates decoded (flags 0), H(m) beside them, the aggregate keys of the rows (profiling event 2), Miller loop and final
// exponentiation into S.verdict; then event 3, the rows of the tuples that go the exact way zeroed and the check counted (k_clo_settle).
BN_HIDDEN int clo_tuple_check(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t t_piece, const ClScratch& S);
// ... and the head of a fallback slice: decode and spread of the items lo .. lo + len (the call's flags), and their candidates of the tuples
// that go the exact way queued in the workspace's h_list / h_cnt and counted
BN_HIDDEN int clo_queue_slice(bn254_ctx* c, hipStream_t s, const ClCall& a, size_t lo, size_t len, const ClScratch& S);
// ... and the stages of that route the optimistic threshold call (bn254_threshold.hip) enqueues one by one, its tuple check being its own:
// rules 1-3 of every share into a.item_status; H(m) and the hash status of the tuples lo .. lo + len into workspace entries 0 .. len; and,
// behind the verdicts, the rows of the tuples that go the exact way zeroed and the check counted (k_clo_settle)
BN_HIDDEN int clo_precheck_all(bn254_ctx* c, hipStream_t s, const ClCall& a, const ClScratch& S);
BN_HIDDEN int clo_load_h(bn254_ctx* c, hipStream_t s, size_t lo, size_t len, const ClScratch& S);
BN_HIDDEN int clo_settle(bn254_ctx* c, hipStream_t s, const ClCall& a, const ClScratch& S);
// the aggregate keys of a device-side QUEUE of tuples on lane pairs (bn254_bitmap_rand.hip: k_bmr_sum_pair_q): lane pair e < *count takes row
// map[e] of d_bits into the Q planes of entry map[e]; rule 2 is the caller's.  n = the most the queue can hold
BN_HIDDEN int launch_bitmap_sum_queued(bn254_ctx* c, hipStream_t s, const uint32_t* d_bits, size_t bm_words, size_t n, bool tables, const uint32_t* map,
                                       const uint32_t* count);
// Compressed G1 input (BN254_FLAG_G1_COMPRESSED; bn254_g1stage.hip, bodies in bn254_g1stage.h).  An entry point that does not take the flag
// refuses it, so that no call reads 33-byte data at a 64-byte stride:
static inline bool g1c_flag(uint32_t flags) { return (flags & BN254_FLAG_G1_COMPRESSED) != 0; }
// ... bytes per G1 item of a call's input array under its flags (what a host form stages)
static inline size_t g1_item_bytes(uint32_t flags) { return g1c_flag(flags) ? 33 : 64; }
// The three steps around a call that takes it.  g1c_reserve: c->g1c_buf for n items (growing it waits for the context's streams: before the
// call's first kernel).  g1c_stage: one lane per item, d_in33 (no alignment) -> the 64 bytes the call reads instead at c->g1c_buf + 64 i and
// the pre-status at g1c_pre(c, n)[i].  g1c_overlay, behind the call: d_status[i] = pre where pre != 0 and the call wrote 6.
BN_HIDDEN int g1c_reserve(bn254_ctx* c, size_t n);
BN_HIDDEN int g1c_stage(bn254_ctx* c, hipStream_t s, const uint8_t* d_in33, size_t n);
BN_HIDDEN int g1c_overlay(bn254_ctx* c, hipStream_t s, size_t n, uint8_t* d_status);
static inline uint8_t* g1c_pre(const bn254_ctx* c, size_t n) { return c->g1c_buf + 64 * n; }
// A *_device entry point under the flag, at its outermost entry and before any slicing: stage the n_items encodings, run(items64) = the same
// call with the flag cleared on the staged items — the existing route, untouched, its own checks included —, then the overlay over d_status.
// live: the call has work (n != 0).  A call without items, or one whose checks will refuse it anyway (no items array, no status array), runs
// on a null items pointer: nothing is staged and nothing read.  Profiling: the staging lies in front of the call's first event.
template <class Run> static inline int g1c_call(bn254_ctx* c, const uint8_t* d_in33, size_t n_items, bool live, uint8_t* d_status, void* stream, Run run) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || n_items > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (!live || !n_items || !d_in33 || !d_status) return run((const uint8_t*)nullptr);
  if (const hipError_t e = hipSetDevice(c->device)) return -(int)e;
  int rc = g1c_reserve(c, n_items);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  if ((rc = g1c_stage(c, s, d_in33, n_items))) return rc;
  if ((rc = run((const uint8_t*)c->g1c_buf))) return rc;
  return g1c_overlay(c, s, n_items, d_status);
}
// ... the same for a call of the collect family (items = the shares or the partials, statuses = a.item_status): run(d) with d = the call on
// the staged items, flag cleared.  cl_stage stages 33 bytes per item under the flag; a host form hands the flag on to its device form.
template <class Run> static inline int cl_g1c_call(bn254_ctx* c, const ClCall& a, void* stream, Run run) {
  return g1c_call(c, a.items, a.n_items, a.n != 0, a.item_status, stream, [&](const uint8_t* items64) {
    ClCall d = a;
    d.items = items64;
    d.flags &= ~BN254_FLAG_G1_COMPRESSED;
    return run(d);
  });
}
// developer hook bn254_debug_fq2_limbs, layout 1 (bn254_pair.hip: k_debug_fq2_limbs_pair): one Fq2 primitive per lane pair on raw limbs; the
// buffers are device memory in the hook's format
BN_HIDDEN int bn254_pair_debug_fq2_limbs(int op, const int32_t* d_in, const int32_t* d_coef, size_t n, int32_t* d_out, uint8_t* d_flags, hipStream_t s);
BN_HIDDEN int launch_encode_g1(bn254_ctx* c, hipStream_t s, size_t n, int px, int inf_plane, uint8_t* out, uint8_t* status_out);
// vectors of G2 points combined column by column (bn254_reshare.hip) run two kernels of other units: the decode of bn254_polyeval.hip — m points
// into its 146 B layout — and the two segment sums of bn254_dealing.hip over terms the caller has written (m terms, n segments by d_seg,
// split by BN254_OPT_COLLECT_WAVE_MIN_SHARES, d_gate as in launch_g2msm)
BN_HIDDEN int launch_pe_decode(hipStream_t s, const uint8_t* d_points, size_t m, int32_t* xy, uint8_t* inf, uint8_t* st);
BN_HIDDEN int launch_g2msm_sums(bn254_ctx* c, hipStream_t s, const G2Jac* terms, const uint8_t* term_st, size_t m, const uint64_t* d_seg, const uint8_t* d_gate,
                                size_t n, uint8_t* d_out, uint8_t* d_status);
