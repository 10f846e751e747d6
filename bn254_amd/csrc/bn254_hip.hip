// libbn254hip.so — HIP kernels for gfx950 (MI355X) + the C ABI declared in include/bn254_hip.h.
//
// Execution model: a batch is processed by a short chain of kernels that hand per-item state to each other
// through an HBM workspace laid out limb-major ("planes"): word k of field element e of item i lives at
//   ws[(e*9 + k) * stride + i]       (9 x 29-bit balanced limbs per field element)
// so a wave reads/writes contiguous bytes per limb (fully coalesced), and the caller-facing byte formats (AoS,
// big-endian) are touched exactly once on the way in/out.  Fq-level work (decoding, hash-to-G1, G1 arithmetic)
// runs one item per lane in this translation unit; everything built on the Fq2 tower (Miller loops, final
// exponentiation, G2 sums and subgroup tests) runs one item per LANE PAIR in bn254_pair.hip, with the
// one-lane-per-item kernels of this file kept behind BN254_OPT_PAIR_LANES = 0.
//
//   batch_verify:  k_decode_g1, k_decode_g2 -> k_hash_init/round/resolve/finish -> k_miller_verify_pair -> k_final_exp_pair
//
// HBM traffic per verify is 225 B of input/output + 2 x ~1 KB of workspace hand-off against ~19 k Montgomery
// products: the path is bound by VALU integer-multiply issue, not by HBM.
#include <hip/hip_runtime.h>
#include <thread>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/bn254_hip.h"
#include "bn254_hash.h"
#include "bn254_io.h"
#include "bn254_pairing.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// decode n G1 points (64 B each) into planes (px, px+1) + inf byte plane; status into st_plane
// (first error wins if `accumulate`)
KERNEL_SMALL void k_decode_g1(const uint8_t* pts, size_t n, uint32_t flags, Ws ws, int px, int inf_plane, int accumulate) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G1Affine p;
  uint8_t st = decode_g1(p, pts + 64 * i, flags);
  if (st != ST_OK) g1_set_generator(p);
  ws_store_g1(ws, px, inf_plane, i, p);
  uint8_t prev = accumulate ? ws_byte(ws, BY_ST_DECODE, i) : (uint8_t)ST_OK;
  ws_byte(ws, BY_ST_DECODE, i) = prev != ST_OK ? prev : st;
}
KERNEL void k_decode_g2(const uint8_t* pts, size_t n, uint32_t flags, Ws ws, int accumulate) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G2Affine q;
  uint8_t st = decode_g2(q, pts + 128 * i, flags);
  if (st != ST_OK) g2_set_generator(q);
  if (flags & FLAG_G2_SUBGROUP_CHECK) {   // wave-uniform branch; every lane runs the ladder
    bool in = g2_in_subgroup(q);
    if (st == ST_OK && !in) { st = ST_INVALID_GROUP_POINT; g2_set_generator(q); }
  }
  ws_store_g2(ws, i, q);
  uint8_t prev = accumulate ? ws_byte(ws, BY_ST_DECODE, i) : (uint8_t)ST_OK;
  ws_byte(ws, BY_ST_DECODE, i) = prev != ST_OK ? prev : st;
}

// Message i of an offsets array: the bytes [off[i], off[i+1]) of a buffer of msgs_len bytes.  A pair that is reversed or
// runs past the buffer — only a *_device caller can hand one over: the host entry points validate their arrays, Rust slices
// cannot express one (/root/reference/src/ecdsa.rs:49) — is hashed as the EMPTY message, never dereferenced, and the item
// reports InvalidLength (5) in its hash status.  msgs_len = UINT64_MAX when the caller did not declare the buffer size
// (bn254_ctx_expect_msgs_len): then only reversed pairs can be caught.
__device__ __forceinline__ bool msg_span(const uint64_t* off, size_t i, uint64_t msgs_len, uint64_t& lo, uint64_t& len) {
  lo = off[i];
  const uint64_t hi = off[i + 1];
  const bool ok = lo <= hi && hi <= msgs_len;
  len = ok ? hi - lo : 0;
  if (!ok) lo = 0;
  return ok;
}
KERNEL_SMALL void k_hash_init(size_t n, Ws ws) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i < n) { ws.h_best[i] = HASH_NONE; ws.h_next[i] = 0; }
  if (i <= HASH_MAX_ROUNDS) ws.h_cnt[i] = (i == 0) ? (uint32_t)n : 0u;
}
KERNEL_SMALL void k_hash_round(const uint8_t* msgs, const uint64_t* off, uint64_t msgs_len, Ws ws, int round, uint32_t width, uint32_t max_ctr) {
  const uint32_t n_act = ws.h_cnt[round];
  if (n_act == 0) return;
  const uint32_t* list = round == 0 ? nullptr : ws.h_list + (size_t)(round & 1) * ws.stride;
  const size_t total = (size_t)n_act * width;
  for (size_t w = (size_t)blockIdx.x * BN_WAVE + threadIdx.x; w < total; w += (size_t)gridDim.x * BN_WAVE) {
    uint32_t slot = (uint32_t)(w % n_act), j = (uint32_t)(w / n_act);
    uint32_t i = list ? list[slot] : slot;
    uint32_t ctr = (uint32_t)ws.h_next[i] + j;
    if (ctr >= max_ctr) continue;                                  // hash.rs:40: counters 0..=254
    uint64_t lo, len;
    msg_span(off, i, msgs_len, lo, len);
    const uint8_t* msg = msgs + lo;
    HashState hs;
    hash_state_init(hs, msg, len);
    if (hash_try_filter(hs, msg, len, ctr)) atomicMin(&ws.h_best[i], ctr);
  }
}
// after a round: messages without a passing counter are queued for the next round (or give up at max_ctr).
// Queue positions: ONE atomic per 1024-slot tile.  An atomic per wave (what `atomicAdd` on a wave-uniform address compiles to anyway:
// the backend already reduces it across the wave) is 262 144 same-address atomics in the first round of configs[4], which the L2 channel
// that owns the counter serialises at ~10 ns each: 3 ms for that one launch, 6.3 ms per 16 Mi step, 99 % wait
// (profiles/r04_m_kernel_stats_hash.csv).  A 1024-lane workgroup counts its survivors through LDS, its first lane reserves the tile's
// range, every survivor takes base + the waves before it + its rank in its own wave.
// Rounds of up to HASH_RESOLVE_TILES_MIN slots keep one wave per 64 slots (k_hash_resolve: a few thousand atomics at most, and no
// workgroup barriers on the latency path of the headline's 65 536-message hash).
// `mark` (HASH_NONE = none): the value a survivor's h_best gets — HASH_TAIL in the wide schedule, whose survivors are finished by the tail
// blocks of k_hash_finish_tail and by nobody else.
KERNEL_SMALL void k_hash_resolve(Ws ws, int round, uint32_t width, uint32_t max_ctr, uint32_t mark) {
  const uint32_t n_act = ws.h_cnt[round];
  if (n_act == 0) return;
  const uint32_t* list = round == 0 ? nullptr : ws.h_list + (size_t)(round & 1) * ws.stride;
  uint32_t* list_out = ws.h_list + (size_t)((round + 1) & 1) * ws.stride;
  const size_t span = (size_t)gridDim.x * BN_WAVE;
  for (size_t base = (size_t)blockIdx.x * BN_WAVE; base < n_act; base += span) {        // wave-uniform trip count: the vote needs every lane
    const size_t slot = base + threadIdx.x;
    bool survivor = false;
    uint32_t i = 0;
    if (slot < n_act) {
      i = list ? list[slot] : (uint32_t)slot;
      if (ws.h_best[i] == HASH_NONE) {
        const uint32_t next = (uint32_t)ws.h_next[i] + width;
        if (next < max_ctr) {                                                             // else hash.rs:62: HashToPointError (k_hash_finish)
          ws.h_next[i] = (uint8_t)next; survivor = true;
          if (mark != HASH_NONE) ws.h_best[i] = mark;
        }
      }
    }
    const uint64_t votes = __ballot(survivor);
    if (votes == 0) continue;
    uint32_t first = 0;
    if (threadIdx.x == 0) first = atomicAdd(&ws.h_cnt[round + 1], (uint32_t)__popcll(votes));
    first = __shfl(first, 0, BN_WAVE);
    if (survivor) list_out[first + (uint32_t)__popcll(votes & ((1ull << threadIdx.x) - 1ull))] = i;
  }
}
#define HASH_RESOLVE_WG 1024
#define HASH_RESOLVE_TILES_MIN ((size_t)1 << 20)
__global__ void __launch_bounds__(HASH_RESOLVE_WG) k_hash_resolve_tiles(Ws ws, int round, uint32_t width, uint32_t max_ctr, uint32_t mark) {
  const uint32_t n_act = ws.h_cnt[round];
  if (n_act == 0) return;
  const uint32_t* list = round == 0 ? nullptr : ws.h_list + (size_t)(round & 1) * ws.stride;
  uint32_t* list_out = ws.h_list + (size_t)((round + 1) & 1) * ws.stride;
  __shared__ uint32_t wave_cnt[HASH_RESOLVE_WG / BN_WAVE];
  __shared__ uint32_t tile_base;
  const unsigned wave = threadIdx.x / BN_WAVE, lane = threadIdx.x % BN_WAVE;
  const size_t span = (size_t)gridDim.x * HASH_RESOLVE_WG;
  for (size_t base = (size_t)blockIdx.x * HASH_RESOLVE_WG; base < n_act; base += span) {    // workgroup-uniform trip count: barriers inside
    const size_t slot = base + threadIdx.x;
    bool survivor = false;
    uint32_t i = 0;
    if (slot < n_act) {
      i = list ? list[slot] : (uint32_t)slot;
      if (ws.h_best[i] == HASH_NONE) {
        const uint32_t next = (uint32_t)ws.h_next[i] + width;
        if (next < max_ctr) {                                                             // else hash.rs:62: HashToPointError (k_hash_finish)
          ws.h_next[i] = (uint8_t)next; survivor = true;
          if (mark != HASH_NONE) ws.h_best[i] = mark;
        }
      }
    }
    const uint64_t votes = __ballot(survivor);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
      for (unsigned w = 0; w < HASH_RESOLVE_WG / BN_WAVE; ++w) { const uint32_t c = wave_cnt[w]; wave_cnt[w] = total; total += c; }   // -> exclusive prefix
      tile_base = total ? atomicAdd(&ws.h_cnt[round + 1], total) : 0u;
    }
    __syncthreads();
    if (survivor) list_out[tile_base + wave_cnt[wave] + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = i;
    __syncthreads();                                                                      // wave_cnt / tile_base are rewritten by the next tile
  }
}
// SMALL batches (n <= HASH_DIRECT_MAX_N): latency, not work, is what counts — the first `width` counters of a message
// (a power of two <= 32, default 32) are tried in as many lanes of one wave with the square root itself (no filter pass
// first: SHA-256 + one exponentiation instead of SHA-256 + Jacobi symbol, then SHA-256 + exponentiation in a second
// kernel), the lowest passing counter writes its point.  A message without one (p = 0.5274^32 = 1.3e-9) is queued as a
// survivor of "round 0" for the ordinary rounds, which start at counter `width` (and cost it a second exponentiation).
KERNEL_SMALL void k_hash_direct(const uint8_t* msgs, const uint64_t* off, uint64_t msgs_len, size_t n, Ws ws, uint32_t width, uint32_t max_ctr, int px,
                                int inf_plane, uint8_t* tries_out) {
  const size_t w = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const size_t i = w / width;
  const uint32_t ctr = (uint32_t)(w % width);
  bool ok = false;
  G1Affine p;
  g1_set_generator(p);
  bool span_ok = true;
  if (i < n && ctr < max_ctr) {
    uint64_t lo, len;
    span_ok = msg_span(off, i, msgs_len, lo, len);
    const uint8_t* msg = msgs + lo;
    HashState hs;
    hash_state_init(hs, msg, len);
    ok = hash_try(p, hs, msg, len, ctr);
  }
  const uint64_t pass = __ballot(ok);
  if (i >= n) return;
  if (!span_ok) {                                                   // the whole counter group of the message agrees
    if (ctr == 0) {
      g1_set_generator(p);
      ws_store_g1(ws, px, inf_plane, i, p);
      ws_byte(ws, BY_ST_HASH, i) = (uint8_t)ST_INVALID_LENGTH;
      if (tries_out) tries_out[i] = 0;
      ws.h_best[i] = HASH_DONE;
    }
    return;
  }
  const uint32_t group = (uint32_t)(pass >> (threadIdx.x & ~(width - 1u))) & (uint32_t)((1ull << width) - 1u);
  if (group != 0) {
    if (ctr == (uint32_t)__builtin_ctz(group)) {                    // hash.rs:40-59: the first counter that yields a point
      ws_store_g1(ws, px, inf_plane, i, p);
      ws_byte(ws, BY_ST_HASH, i) = (uint8_t)ST_OK;
      if (tries_out) tries_out[i] = (uint8_t)(ctr + 1);
      ws.h_best[i] = HASH_DONE;
    }
  } else if (ctr == 0) {
    ws.h_best[i] = HASH_NONE;
    ws.h_next[i] = (uint8_t)width;
    if (width < max_ctr) {
      const uint32_t pos = atomicAdd(&ws.h_cnt[1], 1u);
      (ws.h_list + ws.stride)[pos] = (uint32_t)i;                   // the list that feeds round 1
    }
  }
}
// the point of every message: the even root for its winning counter (or the error status)
__device__ __forceinline__ void hash_finish_item(const uint8_t* msgs, const uint64_t* off, uint64_t msgs_len, size_t i, const Ws& ws, uint32_t max_ctr, int px,
                                                 int inf_plane, uint8_t* tries_out) {
  const uint32_t best = ws.h_best[i];
  if (best == HASH_DONE || best == HASH_TAIL) return;              // k_hash_direct has written it / a tail block of k_hash_finish_tail does
  uint64_t lo, len;
  const bool span_ok = msg_span(off, i, msgs_len, lo, len);
  const uint8_t* msg = msgs + lo;
  HashState hs;
  hash_state_init(hs, msg, len);
  G1Affine p;
  // the filter and the exponentiation agree by construction (Euler's criterion); a disagreement would be
  // reported as an error status, never as a wrong point
  bool ok = span_ok && best != HASH_NONE && hash_try(p, hs, msg, len, best);
  if (!ok) g1_set_generator(p);
  ws_store_g1(ws, px, inf_plane, i, p);
  ws_byte(ws, BY_ST_HASH, i) = ok ? (uint8_t)ST_OK : !span_ok ? (uint8_t)ST_INVALID_LENGTH : (uint8_t)ST_HASH_TO_POINT;
  if (tries_out) tries_out[i] = ok ? (uint8_t)(best + 1) : !span_ok ? (uint8_t)0 : (uint8_t)max_ctr;
}
KERNEL_SMALL void k_hash_finish(const uint8_t* msgs, const uint64_t* off, uint64_t msgs_len, size_t n, Ws ws, uint32_t max_ctr, int px, int inf_plane,
                                uint8_t* tries_out) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  hash_finish_item(msgs, off, msgs_len, i, ws, max_ctr, px, inf_plane, tries_out);
}
// MID-SIZE batches (the wide schedule of launch_hash_rounds): ONE wide filter round leaves few messages without a counter; they must not
// cost everyone else two more dependent rounds.  One launch, two block roles (wave-uniform, by blockIdx as in k_miller_verify_split):
//   blocks [0, nblk_finish)   k_hash_finish for the messages the round decided
//   the blocks behind them    the TAIL: a survivor of the round (list 1, marked HASH_TAIL by the resolve) gets `chunk` lanes of a wave in
//                             k_hash_direct's counter-group form — the square root itself for `chunk` counters at once from h_next on,
//                             the lowest passing counter writes the point; a group without one moves on by `chunk` counters (wave-uniform
//                             loop) until max_ctr, where it reports HashToPointError as k_hash_finish does.
// The tail's grid comes from the expected survivor count; the actual count is read from h_cnt[1] and the groups stride over the list.
// (a function of its own: the tail blocks' square root does not share a register allocation with the finish blocks' inlined one)
__device__ __noinline__ bool hash_try_msg(G1Affine& out, const uint8_t* msg, uint64_t len, uint32_t ctr) {
  HashState hs;
  hash_state_init(hs, msg, len);
  return hash_try(out, hs, msg, len, ctr);
}
KERNEL_SMALL void k_hash_finish_tail(const uint8_t* msgs, const uint64_t* off, uint64_t msgs_len, size_t n, Ws ws, uint32_t max_ctr, int px, int inf_plane,
                                     uint8_t* tries_out, unsigned nblk_finish, uint32_t chunk) {
  if (blockIdx.x < nblk_finish) {
    const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
    if (i < n) hash_finish_item(msgs, off, msgs_len, i, ws, max_ctr, px, inf_plane, tries_out);
    return;
  }
  const uint32_t n_tail = ws.h_cnt[1];
  const uint32_t* list = ws.h_list + ws.stride;
  const uint32_t per_wave = BN_WAVE / chunk, sub = threadIdx.x / chunk, j = threadIdx.x % chunk;
  const size_t span = (size_t)(gridDim.x - nblk_finish) * per_wave;
  for (size_t base = (size_t)(blockIdx.x - nblk_finish) * per_wave; base < n_tail; base += span) {   // wave-uniform trip count: the votes need every lane
    const size_t slot = base + sub;
    const bool live = slot < n_tail;
    uint32_t i = 0, first = 0;
    uint64_t lo = 0, len = 0;
    bool span_ok = true;
    if (live) { i = list[slot]; first = ws.h_next[i]; span_ok = msg_span(off, i, msgs_len, lo, len); }
    const uint8_t* msg = msgs + lo;
    bool open = live && span_ok;                                    // this group still looks for its point
    for (uint32_t k = 0;; k += chunk) {
      const uint32_t ctr = first + k + j;
      bool ok = false;
      G1Affine p;
      if (open && ctr < max_ctr) ok = hash_try_msg(p, msg, len, ctr);   // the hash state is rebuilt per pass (a second pass has p = 1.3e-9 at the default chunk)
      const uint64_t pass = __ballot(ok);
      const uint32_t group = (uint32_t)(pass >> (threadIdx.x & ~(chunk - 1u))) & (uint32_t)((1ull << chunk) - 1u);
      if (group != 0) {
        if (ok && j == (uint32_t)__builtin_ctz(group)) {            // hash.rs:40-59: the first counter that yields a point
          ws_store_g1(ws, px, inf_plane, i, p);
          ws_byte(ws, BY_ST_HASH, i) = (uint8_t)ST_OK;
          if (tries_out) tries_out[i] = (uint8_t)(ctr + 1);
        }
        open = false;
      }
      if (__ballot(open && first + k + chunk < max_ctr) == 0) break;
    }
    if (live && j == 0 && (open || !span_ok)) {                      // counters exhausted (hash.rs:62), or a span that was never dereferenced
      G1Affine p;
      g1_set_generator(p);
      ws_store_g1(ws, px, inf_plane, i, p);
      ws_byte(ws, BY_ST_HASH, i) = span_ok ? (uint8_t)ST_HASH_TO_POINT : (uint8_t)ST_INVALID_LENGTH;
      if (tries_out) tries_out[i] = span_ok ? (uint8_t)max_ctr : (uint8_t)0;
    }
  }
}
// ECDSA::verify Miller loop: f = miller(H(m), pk) * miller(sig, -G2)   (ecdsa.rs:53-57)
// P1 planes hold sig, P2 planes hold H(m), Q planes hold pk.
// With `map` (randomised batch verification, exact re-check of failed groups) lane j works on item
// map[j] for j < *count and leaves at once otherwise.
KERNEL void k_miller_verify(size_t n, Ws ws, const uint32_t* map, const uint32_t* count) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  if (map) { if (i >= *count) return; i = map[i]; }
  G1Affine sig, h;
  G2Affine pk;
  ws_load_g1(ws, PL_P1X, BY_P1_INF, i, sig);
  ws_load_g1(ws, PL_P2X, BY_P2_INF, i, h);
  ws_load_g2(ws, i, pk);
  __shared__ Fp12Slot lds_f[BN_WAVE];
  Fp12& f = lds_f[threadIdx.x].v;
  miller_loop<true, true>(f, h, pk, sig);
  ws_store_f12(ws, i, f);
}
// The same, one PAIRING per lane: the two Miller loops of a verify run in different waves so that a
// 65 536-verify batch puts two waves on every SIMD (two co-resident waves each keep the full
// single-wave issue rate on gfx950).  Workgroups [0, nblk) take pair A = (H(m), pk) with a variable
// twist point, workgroups [nblk, 2 nblk) take pair B = (sig, -G2::one()) through the line table;
// f_A lands at workspace index i, f_B at index f_stride + i; k_final_exp multiplies them.
__device__ __noinline__ void miller_role_a(size_t i, Ws ws) {
  G1Affine h, unused_g1;
  G2Affine pk;
  ws_load_g1(ws, PL_P2X, BY_P2_INF, i, h);
  ws_load_g2(ws, i, pk);
  g1_set_generator(unused_g1);
  Fp12 f;
  miller_loop<true, false>(f, h, pk, unused_g1);
  ws_store_f12(ws, i, f);
}
__device__ __noinline__ void miller_role_b(size_t i, size_t f_stride, Ws ws) {
  G1Affine sig, unused_g1;
  G2Affine unused_g2;
  ws_load_g1(ws, PL_P1X, BY_P1_INF, i, sig);
  g1_set_generator(unused_g1);
  g2_set_generator(unused_g2);
  Fp12 f;
  miller_loop<false, true>(f, unused_g1, unused_g2, sig);
  ws_store_f12(ws, f_stride + i, f);
  ws_byte(ws, BY_ST_DECODE, f_stride + i) = ST_OK;
}
KERNEL void k_miller_verify_split(size_t n, size_t f_stride, unsigned nblk, Ws ws) {
  bool role_b = blockIdx.x >= nblk;     // wave-uniform
  size_t i = (size_t)(blockIdx.x - (role_b ? nblk : 0u)) * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  if (!role_b) miller_role_a(i, ws); else miller_role_b(i, f_stride, ws);
}
// generic single pair per lane: f = miller(P1, Q)
KERNEL void k_miller_var(size_t n, Ws ws) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G1Affine p;
  G2Affine q;
  ws_load_g1(ws, PL_P1X, BY_P1_INF, i, p);
  ws_load_g2(ws, i, q);
  Fp12 f;
  miller_loop<true, false>(f, p, q, p);
  ws_store_f12(ws, i, f);
}
// check_public_keys Miller loop: miller(G1::one(), pk_g2) * miller(pk_g1, -G2)   (ecdsa.rs:80-86)
KERNEL void k_miller_cpk(size_t n, Ws ws) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G1Affine pk1, g;
  G2Affine pk2;
  ws_load_g1(ws, PL_P1X, BY_P1_INF, i, pk1);
  ws_load_g2(ws, i, pk2);
  g1_set_generator(g);
  Fp12 f;
  miller_loop<true, true>(f, g, pk2, pk1);
  ws_store_f12(ws, i, f);
}

// item i: product of the k Miller values f[i*k .. i*k+k), final exponentiation, compare with one.
// status = first decode error among its pairs, else hash error (if use_hash), else 0 / 9.
KERNEL void k_final_exp(size_t n, size_t k, size_t item_stride, size_t pair_stride, Ws ws, int use_hash, uint8_t* gt_out, uint8_t* status_out,
                        int raw_only, size_t base, const uint32_t* map, const uint32_t* count) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  if (map) { if (i >= *count) return; i = map[i]; }   // see k_miller_verify
  // `base`: the factors of item i start at workspace index base + i*item_stride (the per-group values of the
  // randomised batch verification live behind the per-item region); outputs are indexed by i
  // factor j of item i sits at workspace index i*item_stride + j*pair_stride:
  //   pairing API  (k adjacent pairs per item): item_stride = k, pair_stride = 1
  //   split verify (f_A at i, f_B at half + i):  item_stride = 1, pair_stride = half
  // every factor slot carries its own decode status (slots of the B half hold 0)
  Fp12 f, g;
  ws_load_f12(ws, base + i * item_stride, f);
  uint8_t st = ws_byte(ws, BY_ST_DECODE, base + i * item_stride);
  for (size_t j = 1; j < k; ++j) {
    size_t idx = base + i * item_stride + j * pair_stride;
    ws_load_f12(ws, idx, g);
    fp12_mul(f, f, g);
    uint8_t sj = ws_byte(ws, BY_ST_DECODE, idx);
    if (st == ST_OK) st = sj;
  }
  if (st == ST_OK && use_hash) st = ws_byte(ws, BY_ST_HASH, i);
  __shared__ Fp12Slot lds_acc[BN_WAVE];
  if (!raw_only) {
    if (gt_out) final_exponentiation(f, f, lds_acc[threadIdx.x].v);        // canonical Gt: exact exponent
    else final_exponentiation_check(f, f, lds_acc[threadIdx.x].v);          // == one test only: shorter chain
  }
  if (gt_out) encode_fp12(gt_out + 384 * i, f);
  if (status_out) status_out[i] = st != ST_OK ? st : (fp12_is_one(f) ? (uint8_t)ST_OK : (uint8_t)ST_VERIFICATION_FAILED);
}


// the same into the workspace planes of a verify: compressed signatures (33 B) -> P1 planes, compressed public keys
// (65 B, subgroup-checked as G2::from_compressed does) -> Q planes; status as in k_decode_g1 / k_decode_g2
KERNEL_SMALL void k_decompress_g1_ws(const uint8_t* in, size_t n, Ws ws) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G1Affine p;
  uint8_t st = decompress_g1(p, in + 33 * i);
  if (st != ST_OK) g1_set_generator(p);
  ws_store_g1(ws, PL_P1X, BY_P1_INF, i, p);
  ws_byte(ws, BY_ST_DECODE, i) = st;
}
KERNEL void k_decompress_g2_ws(const uint8_t* in, size_t n, Ws ws) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G2Affine q;
  uint8_t st = decompress_g2(q, in + 65 * i);
  if (st != ST_OK) g2_set_generator(q);
  bool in_sub = g2_in_subgroup(q);
  if (st == ST_OK && !in_sub) { st = ST_NOT_MEMBER; g2_set_generator(q); }
  ws_store_g2(ws, i, q);
  uint8_t prev = ws_byte(ws, BY_ST_DECODE, i);
  ws_byte(ws, BY_ST_DECODE, i) = prev != ST_OK ? prev : st;
}
// encode the G1 planes (px, px+1) as uncompressed bytes
KERNEL_SMALL void k_encode_g1(size_t n, Ws ws, int px, int inf_plane, uint8_t* out, uint8_t* status_out) {
  size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  G1Affine p;
  ws_load_g1(ws, px, inf_plane, i, p);
  uint8_t st = ws_byte(ws, BY_ST_HASH, i);
  if (st != ST_OK) p.inf = true;
  encode_g1(out + 64 * i, p);
  if (status_out) status_out[i] = st;
}


// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

int ctx_quiesce(bn254_ctx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->copy_stream));
  HIP_TRY(hipStreamSynchronize(c->kd_stream));
  if (c->last_done_armed) {                         // the last *_device call ran on a caller's stream: wait for the event recorded behind it
    c->last_done_armed = false;
    HIP_TRY(hipEventSynchronize(c->last_done));
  }
  return 0;
}
int ws_reserve(bn254_ctx* c, size_t n) {
  if (n <= c->ws.stride) return 0;
  size_t cap = (n + 255) & ~(size_t)255;
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }     // a *_device call may still be running on a caller's stream, not only on c->stream
  if (c->ws.planes) { HIP_TRY(hipFree(c->ws.planes)); c->ws.planes = nullptr; }
  if (c->ws.bytes) { HIP_TRY(hipFree(c->ws.bytes)); c->ws.bytes = nullptr; }
  if (c->ws.h_best) { HIP_TRY(hipFree(c->ws.h_best)); c->ws.h_best = nullptr; }
  if (c->ws.h_next) { HIP_TRY(hipFree(c->ws.h_next)); c->ws.h_next = nullptr; }
  if (c->ws.h_list) { HIP_TRY(hipFree(c->ws.h_list)); c->ws.h_list = nullptr; }
  c->ws.stride = 0;
  HIP_TRY(hipMalloc((void**)&c->ws.planes, (size_t)N_PLANES * BN_LIMBS * sizeof(int32_t) * cap));
  HIP_TRY(hipMalloc((void**)&c->ws.bytes, (size_t)N_BYTE_PLANES * cap));
  HIP_TRY(hipMalloc((void**)&c->ws.h_best, sizeof(uint32_t) * cap));
  HIP_TRY(hipMalloc((void**)&c->ws.h_next, cap));
  HIP_TRY(hipMalloc((void**)&c->ws.h_list, 2 * sizeof(uint32_t) * cap));
  if (!c->ws.h_cnt) HIP_TRY(hipMalloc((void**)&c->ws.h_cnt, sizeof(uint32_t) * (HASH_MAX_ROUNDS + 1)));
  c->ws.stride = cap;
  return 0;
}
#define WS_BYTES_PER_ITEM ((size_t)N_PLANES * BN_LIMBS * sizeof(int32_t) + N_BYTE_PLANES + sizeof(uint32_t) + 1 + 2 * sizeof(uint32_t))
size_t ws_chunk_for(bn254_ctx* c, size_t n, size_t ws_per_item, bool key_dedup) {
  if (c->max_chunk > 0) return n > (size_t)c->max_chunk ? (size_t)c->max_chunk : 0;
  if (n * ws_per_item <= c->ws.stride && (!key_dedup || (n <= c->kd_items_cap && (size_t)c->kd_max_keys <= c->kd_keys_cap))) return 0;   // already reserved
  // per item: its workspace entries (two with BN254_OPT_SPLIT_MILLER) and the key-dedup words; per call: the dedup's key tables
  const size_t per_item = ws_per_item * WS_BYTES_PER_ITEM + (key_dedup ? KD_BYTES_PER_ITEM : 0);
  const size_t fixed = key_dedup ? (size_t)c->kd_max_keys * KD_BYTES_PER_KEY : 0;
  size_t avail;
  if (c->assume_free_mb > 0) avail = (size_t)c->assume_free_mb << 20;
  else {
    size_t fr = 0, total = 0;
    if (hipSetDevice(c->device) != hipSuccess || hipMemGetInfo(&fr, &total) != hipSuccess) { (void)hipGetLastError(); return 0; }
    avail = fr + c->ws.stride * WS_BYTES_PER_ITEM + c->kd_items_cap * KD_BYTES_PER_ITEM + c->kd_keys_cap * KD_BYTES_PER_KEY;   // growing frees the present buffers first
  }
  const size_t need = ((n + 255) & ~(size_t)255) * per_item + fixed;
  if (need <= avail / 10 * 9) return 0;
  const size_t room = avail / 10 * 8 > fixed ? avail / 10 * 8 - fixed : 0;
  size_t chunk = room / per_item;
  chunk &= ~(size_t)65535;
  if (chunk == 0) chunk = room / per_item & ~(size_t)255;   // a very small device share: whatever fits (a failure to allocate is then reported as before)
  // the key tables leave no room for a slice that would still take the dedup route: price the generic route instead (its slices are then too
  // small for the dedup, or kd_reserve finds no room for the tables and the slice takes the generic loop, KD_NO_ROOM) — never "do not slice"
  if (key_dedup && (chunk == 0 || route_for(c, chunk).miller != BN_ML_LANE_PAIRS)) return ws_chunk_for(c, n, ws_per_item, false);
  return chunk && chunk < n ? chunk : 0;
}
// the key-dedup buffers (bn254_ws.h: KeyDedup) for n items and the context's max_keys, grown on demand
#define KD_NO_ROOM 1
static int kd_reserve(bn254_ctx* c, size_t n, KeyDedup& kd) {
  size_t slots = 1;
  while (slots < 2 * n) slots <<= 1;
  const size_t keys = (size_t)c->kd_max_keys;
  if (n > c->kd_items_cap || keys > c->kd_keys_cap) {
    const size_t items_cap = n > c->kd_items_cap ? ((n + 255) & ~(size_t)255) : c->kd_items_cap;
    const size_t keys_cap = keys > c->kd_keys_cap ? keys : c->kd_keys_cap;
    { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
    if (c->kd_buf) { HIP_TRY(hipFree(c->kd_buf)); c->kd_buf = nullptr; }
    c->kd_items_cap = c->kd_keys_cap = 0;
    c->kd_ctl = nullptr;
    c->kd_lines_last = nullptr;
    c->kd_fold_last = nullptr;
    c->kd_cache_valid = false;                         // the cache lived in the freed buffer: the next call starts from an empty one
    if (hipMalloc((void**)&c->kd_buf, items_cap * KD_BYTES_PER_ITEM + keys_cap * KD_BYTES_PER_KEY + 512) != hipSuccess) {
      (void)hipGetLastError();                       // no room for the tables: this call takes the generic route (the caller sees no error)
      c->kd_buf = nullptr;
      return KD_NO_ROOM;
    }
    c->kd_items_cap = items_cap;
    c->kd_keys_cap = keys_cap;
  }
  size_t slots_cap = 1;
  while (slots_cap < 2 * c->kd_items_cap) slots_cap <<= 1;           // slot arrays sized for the capacity: <= 4 x items_cap words each
  uint8_t* p = c->kd_buf;
  auto take = [&](size_t bytes) { uint8_t* r = p; p += (bytes + 15) & ~(size_t)15; return r; };
  kd.table = (uint32_t*)take(slots_cap * 4);
  kd.slot_id = (uint32_t*)take(slots_cap * 4);
  kd.slot_of = (uint32_t*)take(c->kd_items_cap * 4);
  kd.key_idx = (uint32_t*)take(c->kd_items_cap * 4);
  kd.lines = (int32_t*)take(c->kd_keys_cap * BN_N_FIXED_LINES * BN_KEY_LINE_WORDS * 4);
  kd.fold = (int32_t*)take(c->kd_keys_cap * KD_FOLD_KEY_WORDS * 4);
  kd.c2 = kd.fold;                                                   // a key's raw c2 while it is built, its folded rows afterwards (bn254_ws.h)
  kd.rep = (uint32_t*)take(c->kd_keys_cap * 4);
  kd.ctl = (uint32_t*)take(KD_CTL_WORDS * 4);
  c->kd_ctl = kd.ctl;
  kd.st = take(c->kd_keys_cap);
  kd.inf = take(c->kd_keys_cap);
  kd.row_of = (uint32_t*)take(c->kd_keys_cap * 4);
  kd.build_row = (uint32_t*)take(c->kd_keys_cap * 4);
  kd.build_rep = (uint32_t*)take(c->kd_keys_cap * 4);
  kd.c_keys = (uint32_t*)take(c->kd_keys_cap * 128);
  size_t index_slots = 1;
  while (index_slots < 2 * keys) index_slots <<= 1;                  // at most half full: < 4 x keys_cap words
  kd.c_index = (uint32_t*)take(4 * c->kd_keys_cap * 4);
  kd.c_state = (uint32_t*)take(4);
  kd.index_mask = (uint32_t)(index_slots - 1);
  c->kd_lines_last = kd.lines; c->kd_fold_last = kd.fold; c->kd_rep_last = kd.rep; c->kd_st_last = kd.st; c->kd_inf_last = kd.inf; c->kd_row_of_last = kd.row_of;
  kd.slot_mask = (uint32_t)(slots - 1);
  kd.hash_mask = c->kd_hash_bits > 0 && c->kd_hash_bits < 32 ? (1u << c->kd_hash_bits) - 1 : 0xFFFFFFFFu;
  kd.max_keys = (uint32_t)keys;
  kd.min_mult = (uint32_t)c->kd_min_mult;
  return 0;
}
int scratch_reserve(bn254_ctx* c, uint8_t** buf, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return 0;
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  if (*buf) { HIP_TRY(hipFree(*buf)); *buf = nullptr; *cap = 0; }
  const size_t grown = (bytes + 4095) & ~(size_t)4095;
  HIP_TRY(hipMalloc((void**)buf, grown));
  *cap = grown;
  return 0;
}
int stage_reserve(bn254_ctx* c, int slot, size_t bytes) {
  if (bytes <= c->stage_cap[slot]) return 0;
  HIP_TRY(hipSetDevice(c->device));
  return scratch_reserve(c, &c->stage[slot], &c->stage_cap[slot], bytes);
}
uint8_t* HostStaging::out(int slot, size_t bytes, void* host) {
  if (!rc) rc = stage_reserve(c, slot, bytes);
  if (rc) return nullptr;
  if (host) copy_back(host, c->stage[slot], bytes);
  return c->stage[slot];
}
uint8_t* HostStaging::in(int slot, const void* host, size_t bytes) {
  uint8_t* d = out(slot, bytes ? bytes : 1);
  if (d && bytes) check(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->stream));
  return rc ? nullptr : d;
}
void HostStaging::copy_back(void* host, const void* dev, size_t bytes) {
  if (!host || !bytes) return;
  if (n_back == (int)(sizeof back / sizeof back[0])) { check(hipErrorInvalidValue); return; }   // more outputs than any entry point has
  back[n_back++] = {host, dev, bytes};
}
hipError_t HostStaging::drain() {
  finished = true;
  const hipError_t e = hipStreamSynchronize(c->stream);
  const hipError_t e_copy = hipStreamSynchronize(c->copy_stream);   // verify_host_overlapped's second stream (idle for every other call)
  return e != hipSuccess ? e : e_copy;
}
int HostStaging::finish() {
  for (int i = 0; i < n_back && !rc; ++i) check(hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, c->stream));
  const hipError_t e = drain();
  return rc ? rc : -(int)e;
}
// a pool outside the numbered slots (the comb table of the G2 generator): allocated once, never resized in practice
int pool_reserve_one(bn254_ctx* c, Pool* p, size_t n_fp, size_t entries) {
  if (entries <= p->stride) return 0;
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  if (p->planes) { HIP_TRY(hipFree(p->planes)); p->planes = nullptr; }
  if (p->st) { HIP_TRY(hipFree(p->st)); p->st = nullptr; }
  p->stride = 0;
  const size_t cap = (entries + 255) & ~(size_t)255;
  p->g2 = n_fp == 4 ? 1u : 0u;
  HIP_TRY(hipMalloc((void**)&p->planes, (n_fp / 2) * BN_POOL_HALF_WORDS * sizeof(int32_t) * cap));
  HIP_TRY(hipMalloc((void**)&p->st, cap));
  p->stride = cap;
  return 0;
}
int pool_reserve(bn254_ctx* c, int which, size_t n_fp, size_t entries) {
  Pool& p = c->pool[which];
  if (entries <= p.stride && c->pool_fp[which] == n_fp) return 0;
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  if (p.planes) { HIP_TRY(hipFree(p.planes)); p.planes = nullptr; }
  if (p.st) { HIP_TRY(hipFree(p.st)); p.st = nullptr; }
  p.stride = 0;
  size_t cap = (entries + 255) & ~(size_t)255;
  p.g2 = n_fp == 4 ? 1u : 0u;                       // record layout: bn254_ws.h
  HIP_TRY(hipMalloc((void**)&p.planes, (n_fp / 2) * BN_POOL_HALF_WORDS * sizeof(int32_t) * cap));
  HIP_TRY(hipMalloc((void**)&p.st, cap));
  p.stride = cap;
  c->pool_fp[which] = n_fp;
  return 0;
}

// G2 decoding: with the subgroup test requested (one 63-bit ladder on the twist per point) it runs on lane pairs
int launch_decode_g2(bn254_ctx* c, hipStream_t s, const uint8_t* d_pts, size_t n, uint32_t flags, int accumulate) {
  if (c->pair_lanes && (flags & FLAG_G2_SUBGROUP_CHECK)) {
    if (route_lane_machine_helpers(c, n)) {
      // the smallest batches: decode without the test, then the test with its ladder in the lane machine's level tables
      k_decode_g2<<<grid_for(n), BN_WAVE, 0, s>>>(d_pts, n, flags & ~(uint32_t)FLAG_G2_SUBGROUP_CHECK, c->ws, accumulate);
      return bn254_lm_g2_subgroup(n, c->ws, s);
    }
    return bn254_pair_decode_g2(d_pts, n, flags, c->ws, accumulate, s);
  }
  k_decode_g2<<<grid_for(n), BN_WAVE, 0, s>>>(d_pts, n, flags, c->ws, accumulate);
  return 0;
}

// width of the one round of the wide schedule: the smallest from 4 on (at most 8) with which the launch behind it — n / 64 finish waves and one
// 32-lane group per expected survivor — stays within one wave per SIMD, so that every square root runs at a lone wave's rate in one pass.
// Measured at 16 385 / 32 768 (profiles/hash_schedule_sweep.jsonl): widths 4 / 6 are the fastest, and they are what this rule gives.
static uint32_t hash_wide_width(size_t n) {
  double survivors = (double)n * 0.5274 * 0.5274 * 0.5274 * 0.5274;
  uint32_t w = 4;
  for (; w < 8 && (double)n / BN_WAVE + survivors * HASH_TAIL_CHUNK_DEFAULT / BN_WAVE > (double)HASH_WIDE_WAVES; ++w) survivors *= 0.5274;
  return w;
}
// The schedule (widths, grid sizes) is fixed on the host from the EXPECTED survivor counts
// (p_fail = 0.5274 per try); the kernels read the actual counts from device memory and use grid-stride
// loops, so a wrong estimate costs time, never correctness.  No host synchronisation.
int launch_hash_rounds(bn254_ctx* c, hipStream_t s, const uint8_t* d_msgs, const uint64_t* d_off, size_t n, int px, int inf_plane,
                              uint8_t* d_tries, int mark_finish) {           // mark_finish: profiling event recorded in front of k_hash_finish
  const uint32_t max_ctr = c->hash_max_tries ? (uint32_t)c->hash_max_tries : 255u;
  const uint64_t msgs_len = c->msgs_len_call;   // bn254_ctx_expect_msgs_len, taken by the entry point's MsgsLenScope
  k_hash_init<<<grid_for(n > HASH_MAX_ROUNDS + 1 ? n : HASH_MAX_ROUNDS + 1), BN_WAVE, 0, s>>>(n, c->ws);
  if (n <= HASH_DIRECT_MAX_N && c->hash_direct_width > 0) {
    const uint32_t width = (uint32_t)c->hash_direct_width;
    k_hash_direct<<<grid_for(n * width), BN_WAVE, 0, s>>>(d_msgs, d_off, msgs_len, n, c->ws, width, max_ctr, px, inf_plane, d_tries);
    if (max_ctr > width)                 // the (rare) survivors: every remaining counter at once (grid-stride beyond 64 of them)
      k_hash_round<<<grid_for(64 * (max_ctr - width)), BN_WAVE, 0, s>>>(d_msgs, d_off, msgs_len, c->ws, 1, max_ctr - width, max_ctr);
    if (mark_finish >= 0 && c->profiling) HIP_TRY(hipEventRecord(c->ev[mark_finish], s));
    k_hash_finish<<<grid_for(n), BN_WAVE, 0, s>>>(d_msgs, d_off, msgs_len, n, c->ws, max_ctr, px, inf_plane, d_tries);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  if (n > HASH_DIRECT_MAX_N && (c->hash_schedule == 2 || (c->hash_schedule == 0 && n <= HASH_WIDE_MAX_N))) {
    // the wide schedule: init, ONE round of width W0, resolve, finish + tail side by side (k_hash_finish_tail)
    uint32_t w0 = c->hash_wide_width ? (uint32_t)c->hash_wide_width : hash_wide_width(n);
    if (w0 > max_ctr) w0 = max_ctr;
    size_t lanes = n * w0;
    if (lanes > HASH_MAX_GRID_LANES) lanes = HASH_MAX_GRID_LANES;
    k_hash_round<<<grid_for(lanes), BN_WAVE, 0, s>>>(d_msgs, d_off, msgs_len, c->ws, 0, w0, max_ctr);
    if (n > HASH_RESOLVE_TILES_MIN) {
      size_t tiles = (n + HASH_RESOLVE_WG - 1) / HASH_RESOLVE_WG;
      if (tiles > 16384) tiles = 16384;
      k_hash_resolve_tiles<<<(unsigned)tiles, HASH_RESOLVE_WG, 0, s>>>(c->ws, 0, w0, max_ctr, HASH_TAIL);
    } else {
      k_hash_resolve<<<grid_for(n), BN_WAVE, 0, s>>>(c->ws, 0, w0, max_ctr, HASH_TAIL);
    }
    double pf = 1.0;
    for (uint32_t t = 0; t < w0 && pf > 1e-12; ++t) pf *= 0.5274;
    double bound = (double)n * pf * 1.25 + 256.0;           // generous estimate of the survivors, as for the rounds below
    if (bound > (double)n) bound = (double)n;
    const uint32_t chunk = (uint32_t)c->hash_tail_chunk;
    size_t tail_blocks = ((size_t)bound * chunk + BN_WAVE - 1) / BN_WAVE;
    if (tail_blocks > HASH_TAIL_MAX_BLOCKS) tail_blocks = HASH_TAIL_MAX_BLOCKS;   // the groups stride over the list beyond
    if (mark_finish >= 0 && c->profiling) HIP_TRY(hipEventRecord(c->ev[mark_finish], s));
    const unsigned nblk = grid_for(n);
    k_hash_finish_tail<<<nblk + (unsigned)tail_blocks, BN_WAVE, 0, s>>>(d_msgs, d_off, msgs_len, n, c->ws, max_ctr, px, inf_plane, d_tries, nblk, chunk);
    HIP_TRY(hipGetLastError());
    return 0;
  }
  double expect = (double)n;
  uint32_t consumed = 0;
  for (int round = 0; round < HASH_MAX_ROUNDS && consumed < max_ctr; ++round) {
    bool last = round == HASH_MAX_ROUNDS - 1;
    double lanes_per_msg = (double)HASH_TARGET_LANES / (expect < 1.0 ? 1.0 : expect);
    uint32_t width = lanes_per_msg < 2.0 ? 1u : (uint32_t)lanes_per_msg;
    if (width > max_ctr - consumed || last) width = max_ctr - consumed;
    double bound = expect * 1.25 + 256.0;                 // generous estimate of the survivors
    if (bound > (double)n) bound = (double)n;
    size_t lanes = (size_t)(bound * width);
    if (lanes > HASH_MAX_GRID_LANES) lanes = HASH_MAX_GRID_LANES;   // grid-stride loops cover the rest
    k_hash_round<<<grid_for(lanes), BN_WAVE, 0, s>>>(d_msgs, d_off, msgs_len, c->ws, round, width, max_ctr);
    if ((size_t)bound > HASH_RESOLVE_TILES_MIN) {
      size_t tiles = ((size_t)bound + HASH_RESOLVE_WG - 1) / HASH_RESOLVE_WG;
      if (tiles > 16384) tiles = 16384;                     // grid-stride beyond
      k_hash_resolve_tiles<<<(unsigned)tiles, HASH_RESOLVE_WG, 0, s>>>(c->ws, round, width, max_ctr, HASH_NONE);
    } else {
      k_hash_resolve<<<grid_for((size_t)bound), BN_WAVE, 0, s>>>(c->ws, round, width, max_ctr, HASH_NONE);
    }
    consumed += width;
    double pf = 1.0;
    for (uint32_t t = 0; t < width && pf > 1e-12; ++t) pf *= 0.5274;
    expect *= pf;
  }
  if (mark_finish >= 0 && c->profiling) HIP_TRY(hipEventRecord(c->ev[mark_finish], s));
  k_hash_finish<<<grid_for(n), BN_WAVE, 0, s>>>(d_msgs, d_off, msgs_len, n, c->ws, max_ctr, px, inf_plane, d_tries);
  HIP_TRY(hipGetLastError());
  return 0;
}

// launchers for the other translation units (bn254_host.h)
int launch_decode_g1(bn254_ctx* c, hipStream_t s, const uint8_t* d_pts, size_t n, uint32_t flags, int px, int inf_plane, int accumulate) {
  k_decode_g1<<<grid_for(n), BN_WAVE, 0, s>>>(d_pts, n, flags, c->ws, px, inf_plane, accumulate);
  return 0;
}
int launch_miller_var_lane(bn254_ctx* c, hipStream_t s, size_t n) {
  k_miller_var<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws);
  return 0;
}
int launch_miller_verify_lane(bn254_ctx* c, hipStream_t s, size_t n, const uint32_t* map, const uint32_t* count) {
  k_miller_verify<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws, map, count);
  return 0;
}
int launch_final_exp_lane(bn254_ctx* c, hipStream_t s, size_t n, size_t k, size_t item_stride, size_t pair_stride, int use_hash, uint8_t* gt_out,
                          uint8_t* status_out, int raw_only, size_t base, const uint32_t* map, const uint32_t* count) {
  k_final_exp<<<grid_for(n), BN_WAVE, 0, s>>>(n, k, item_stride, pair_stride, c->ws, use_hash, gt_out, status_out, raw_only, base, map, count);
  return 0;
}
int launch_encode_g1(bn254_ctx* c, hipStream_t s, size_t n, int px, int inf_plane, uint8_t* out, uint8_t* status_out) {
  k_encode_g1<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws, px, inf_plane, out, status_out);
  return 0;
}

extern "C" {

const char* bn254_version(void) { return "bn254-mi355x 0.7 (gfx950; 9x29-bit balanced Montgomery limbs; verify on lane pairs, batches <= 16384 on lane octets with wave roles; bn254_mgpu_*: all the GPUs of a node behind one handle)"; }

int bn254_ctx_create(int hip_device, bn254_ctx** out) {
  if (!out) return BN254_E_BAD_ARGUMENT;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) return BN254_E_NO_DEVICE;   // no CPU fallback, by design
  if (hip_device < 0 || hip_device >= count) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(hip_device));
  bn254_ctx* c = new (std::nothrow) bn254_ctx();
  if (!c) return BN254_E_BAD_ARGUMENT;
  memset(c, 0, sizeof *c);
  c->pair_lanes = 1;
  c->rand_min_batch = RAND_MIN_BATCH_DEFAULT;
  c->agg_rand_min_pairs = AGG_RAND_MIN_PAIRS_DEFAULT;
  c->agg_rand_group_pairs = AGG_RAND_GROUP_PAIRS_DEFAULT;
  c->bmr_min_tuples = BITMAP_RAND_MIN_TUPLES_DEFAULT;
  c->bmr_group_tuples = BITMAP_RAND_GROUP_TUPLES_DEFAULT;
  c->bmr_max_keys = BITMAP_RAND_MAX_KEYS_DEFAULT;
  c->collect_wave_min = COLLECT_WAVE_MIN_SHARES_DEFAULT;
  c->pe_wave_min = POLY_EVAL_WAVE_MIN_COEFFS_DEFAULT;
  c->collect_rand_min_shares = COLLECT_RAND_MIN_SHARES_DEFAULT;
  c->collect_rand_min_per_key = COLLECT_RAND_MIN_PER_KEY_DEFAULT;
  c->collect_opt_min_shares = COLLECT_OPT_MIN_SHARES_DEFAULT;
  c->collect_opt_min_tuple_shares = COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT;
  c->merge_wave_min = MERGE_WAVE_MIN_PARTS_DEFAULT;
  c->merge_opt_min_parts = MERGE_OPT_MIN_PARTS_DEFAULT;
  c->th_opt_min_shares = THRESHOLD_OPT_MIN_SHARES_DEFAULT;
  c->trio_max_batch = TRIO_MAX_BATCH_DEFAULT;
  c->hash_direct_width = HASH_DIRECT_WIDTH_DEFAULT;
  c->hash_tail_chunk = HASH_TAIL_CHUNK_DEFAULT;
  c->trio_wave_roles = TRIO_WAVE_ROLES_DEFAULT;
  c->agg_subset_min_tuples = AGG_SUBSET_MIN_TUPLES_DEFAULT;
  c->agg_sort_by_msg = 1;
  c->agg_t4_route = 0;
  c->agg_wide_min_tuples = AGG_WIDE_MIN_TUPLES_DEFAULT;
  c->pinned_staging = PINNED_STAGING_DEFAULT;
  // the small-batch kernels ask for up to 156 KB of dynamic LDS per workgroup: on a part that cannot hold one, step down
  // (eight wave roles -> four -> lane groups -> lane pairs only) instead of failing at the first launch
  c->fits_w8 = bn254_quad_fits_device(1); c->fits_quad = bn254_quad_fits_device(0); c->fits_trio = bn254_trio_fits_device();
  if (c->trio_wave_roles == 2 && !c->fits_w8) c->trio_wave_roles = 1;
  if (c->trio_wave_roles == 1 && !c->fits_quad) c->trio_wave_roles = 0;
  if (!c->fits_trio) c->trio_max_batch = 0;
  c->nonet_max_batch = bn254_nonet_fits_device() ? NONET_MAX_BATCH_DEFAULT : 0;
  c->lm_max_batch = bn254_lm_fits_device() ? LM_MAX_BATCH_DEFAULT : 0;
  c->nonet_wide = 1;
  c->g2_fixed_base = 1;
  c->key_dedup = 1;
  c->kd_max_keys = KEY_DEDUP_MAX_KEYS_DEFAULT;
  c->kd_min_mult = KEY_DEDUP_MIN_MULT_DEFAULT;
  c->kd_fold = KEY_DEDUP_FOLD_DEFAULT;
  c->kd_cache = 1;
  c->bm_table_max_keys = BITMAP_TABLE_MAX_KEYS_DEFAULT;
  c->device = hip_device;
  hipError_t err = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&c->last_done, hipEventDisableTiming);
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&c->kd_stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&c->kd_fork, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&c->kd_join, hipEventDisableTiming);
  if (err == hipSuccess) err = hipEventCreateWithFlags(&c->kd_done, hipEventDisableTiming);
  for (int i = 0; i < 5 && err == hipSuccess; ++i) err = hipEventCreate(&c->ev[i]);
  if (err != hipSuccess) {
    if (c->kd_done) (void)hipEventDestroy(c->kd_done);
    if (c->kd_join) (void)hipEventDestroy(c->kd_join);
    if (c->kd_fork) (void)hipEventDestroy(c->kd_fork);
    if (c->kd_stream) (void)hipStreamDestroy(c->kd_stream);
    if (c->last_done) (void)hipEventDestroy(c->last_done);
    for (int i = 0; i < 5; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->copy_done) (void)hipEventDestroy(c->copy_done);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return -(int)err;
  }
  *out = c;
  return 0;
}
void bn254_ctx_destroy(bn254_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)ctx_quiesce(c);                               // own streams + the end of the last call on a caller's stream
  if (c->ws.planes) (void)hipFree(c->ws.planes);
  if (c->ws.bytes) (void)hipFree(c->ws.bytes);
  if (c->ws.h_best) (void)hipFree(c->ws.h_best);
  if (c->ws.h_next) (void)hipFree(c->ws.h_next);
  if (c->ws.h_list) (void)hipFree(c->ws.h_list);
  if (c->ws.h_cnt) (void)hipFree(c->ws.h_cnt);
  if (c->ws.clk) (void)hipFree(c->ws.clk);
  if (c->pin) (void)hipHostFree(c->pin);
  for (int i = 0; i < 8; ++i) { if (c->pool[i].planes) (void)hipFree(c->pool[i].planes); if (c->pool[i].st) (void)hipFree(c->pool[i].st); }
  if (c->g2_comb.planes) (void)hipFree(c->g2_comb.planes);
  if (c->g2_comb.st) (void)hipFree(c->g2_comb.st);
  if (c->g1_comb.planes) (void)hipFree(c->g1_comb.planes);
  if (c->g1_comb.st) (void)hipFree(c->g1_comb.st);
  for (int i = 0; i < 8; ++i) if (c->stage[i]) (void)hipFree(c->stage[i]);
  if (c->key_lines) (void)hipFree(c->key_lines);
  if (c->key_xy) (void)hipFree(c->key_xy);
  if (c->key_st) (void)hipFree(c->key_st);
  if (c->key_inf) (void)hipFree(c->key_inf);
  if (c->aggd_buf) (void)hipFree(c->aggd_buf);
  if (c->aggr_buf) (void)hipFree(c->aggr_buf);
  if (c->aggr_stats) (void)hipFree(c->aggr_stats);
  if (c->bmr_buf) (void)hipFree(c->bmr_buf);
  if (c->collect_buf) (void)hipFree(c->collect_buf);
  if (c->kd_buf) (void)hipFree(c->kd_buf);
  if (c->bm_bad) (void)hipFree(c->bm_bad);
  if (c->bm_tab) (void)hipFree(c->bm_tab);
  if (c->bw_tab) (void)hipFree(c->bw_tab);
  if (c->pop_buf) (void)hipFree(c->pop_buf);
  if (c->th_buf) (void)hipFree(c->th_buf);
  if (c->g1c_buf) (void)hipFree(c->g1c_buf);
  if (c->gk_lines) (void)hipFree(c->gk_lines);
  if (c->gk_xy) (void)hipFree(c->gk_xy);
  if (c->gk_st) (void)hipFree(c->gk_st);
  if (c->gk_inf) (void)hipFree(c->gk_inf);
  for (int i = 0; i < 5; ++i) (void)hipEventDestroy(c->ev[i]);
  (void)hipEventDestroy(c->kd_fork);
  (void)hipEventDestroy(c->kd_join);
  (void)hipEventDestroy(c->kd_done);
  (void)hipStreamDestroy(c->kd_stream);
  (void)hipEventDestroy(c->copy_done);
  (void)hipEventDestroy(c->last_done);
  (void)hipStreamSynchronize(c->copy_stream);
  (void)hipStreamDestroy(c->copy_stream);
  (void)hipStreamDestroy(c->stream);
  delete c;
}
int bn254_ctx_reserve(bn254_ctx* c, size_t n) { return c ? ws_reserve(c, n) : BN254_E_BAD_ARGUMENT; }
int bn254_ctx_reserve_host(bn254_ctx* c, size_t n, size_t msg_bytes) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  int rc = ws_reserve(c, n);
  const size_t need[5] = {msg_bytes ? msg_bytes : 1, (n + 1) * sizeof(uint64_t), n * 64, n * 128, n ? n : 1};
  for (int slot = 0; slot < 5 && !rc; ++slot) rc = stage_reserve(c, slot, need[slot]);
  return rc;
}
int bn254_ctx_synchronize(bn254_ctx* c) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}
int bn254_ctx_expect_msgs_len(bn254_ctx* c, uint64_t msgs_len) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  c->msgs_len_next = msgs_len;
  c->msgs_len_declared = 1;
  return 0;
}
int bn254_ctx_set_profiling(bn254_ctx* c, int enabled) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  c->profiling = enabled;
  c->ev_valid = 0;
  return 0;
}
int bn254_ctx_set_option(bn254_ctx* c, int option, int value) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  if (option == BN254_OPT_SPLIT_MILLER) { c->split_miller = value; return 0; }
  if (option == BN254_OPT_PAIR_LANES) { c->pair_lanes = value != 0; return 0; }
  if (option == BN254_OPT_RAND_MIN_BATCH) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->rand_min_batch = value; return 0; }
  if (option == BN254_OPT_RAND_ITEMS_PER_LANE) { if (value < 0 || value > 2) return BN254_E_BAD_ARGUMENT; c->rand_items_per_lane = value; return 0; }
  if (option == BN254_OPT_AGG_SUBSET_MIN_TUPLES) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->agg_subset_min_tuples = value; return 0; }
  if (option == BN254_OPT_TRIO_MAX_BATCH) {
    if (value < 0 || (value > 0 && !c->fits_trio)) return BN254_E_BAD_ARGUMENT;
    c->trio_max_batch = value;
    return 0;
  }
  if (option == BN254_OPT_TRIO_WAVE_ROLES) {
    if (value < 0 || value > 2 || (value == 2 && !c->fits_w8) || (value == 1 && !c->fits_quad)) return BN254_E_BAD_ARGUMENT;
    c->trio_wave_roles = value;
    return 0;
  }
  if (option == BN254_OPT_HASH_DIRECT_WIDTH) {
    if (value < 0 || value > 32 || (value & (value - 1))) return BN254_E_BAD_ARGUMENT;
    c->hash_direct_width = value;
    return 0;
  }
  if (option == BN254_OPT_HASH_SCHEDULE) { if (value < 0 || value > 2) return BN254_E_BAD_ARGUMENT; c->hash_schedule = value; return 0; }
  if (option == BN254_OPT_HASH_WIDE_WIDTH) { if (value < 0 || value > 64) return BN254_E_BAD_ARGUMENT; c->hash_wide_width = value; return 0; }
  if (option == BN254_OPT_HASH_TAIL_CHUNK) {
    if (value < 2 || value > 32 || (value & (value - 1))) return BN254_E_BAD_ARGUMENT;
    c->hash_tail_chunk = value;
    return 0;
  }
  if (option == BN254_OPT_NONET_MAX_BATCH) {
    HIP_TRY(hipSetDevice(c->device));                 // the fits query asks the CURRENT device
    if (value < 0 || (value > 0 && !bn254_nonet_fits_device())) return BN254_E_BAD_ARGUMENT;
    c->nonet_max_batch = value;
    return 0;
  }
  if (option == BN254_OPT_NONET_WIDE) { c->nonet_wide = value != 0; return 0; }
  if (option == BN254_OPT_LM_MAX_BATCH) {
    HIP_TRY(hipSetDevice(c->device));                 // the fits query asks the CURRENT device
    if (value < 0 || (value > 0 && !bn254_lm_fits_device())) return BN254_E_BAD_ARGUMENT;
    c->lm_max_batch = value;
    return 0;
  }
  if (option == BN254_OPT_PINNED_STAGING) { if (value < 0 || value > 16) return BN254_E_BAD_ARGUMENT; c->pinned_staging = value; return 0; }
  if (option == BN254_OPT_AGG_SORT_BY_MSG) { c->agg_sort_by_msg = value != 0; return 0; }
  if (option == BN254_OPT_AGG_T4_ROUTE) { if (value < 0 || value > 1) return BN254_E_BAD_ARGUMENT; c->agg_t4_route = value; return 0; }
  if (option == BN254_OPT_AGG_WIDE_MIN_TUPLES) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->agg_wide_min_tuples = value; return 0; }
  if (option == BN254_OPT_CLOCK_PROBE) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    if (value && !c->ws.clk) {
      HIP_TRY(hipMalloc((void**)&c->ws.clk, sizeof(unsigned long long) * 3 * BN_CLK_MAX_WG * 2));
      HIP_TRY(hipMemset(c->ws.clk, 0, sizeof(unsigned long long) * 3 * BN_CLK_MAX_WG * 2));
    } else if (!value && c->ws.clk) {
      HIP_TRY(hipFree(c->ws.clk));
      c->ws.clk = nullptr;
    }
    return 0;
  }
  if (option == BN254_OPT_HASH_MAX_TRIES) { if (value < 0 || value > 255) return BN254_E_BAD_ARGUMENT; c->hash_max_tries = value; return 0; }
  if (option == BN254_OPT_G2_FIXED_BASE) { c->g2_fixed_base = value != 0; return 0; }
  if (option == BN254_OPT_MAX_CHUNK) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->max_chunk = value; return 0; }
  if (option == BN254_OPT_ASSUME_FREE_MB) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->assume_free_mb = value; return 0; }
  if (option == BN254_OPT_KEY_DEDUP) { if (value < 0 || value > 1) return BN254_E_BAD_ARGUMENT; c->key_dedup = value; return 0; }
  if (option == BN254_OPT_KEY_DEDUP_MAX_KEYS) { if (value < 0 || value > KEY_DEDUP_MAX_KEYS_LIMIT) return BN254_E_BAD_ARGUMENT; c->kd_max_keys = value; return 0; }
  if (option == BN254_OPT_KEY_DEDUP_MIN_MULT) { if (value < 1) return BN254_E_BAD_ARGUMENT; c->kd_min_mult = value; return 0; }
  if (option == BN254_OPT_KEY_DEDUP_FOLD) { if (value < 0 || value > 2) return BN254_E_BAD_ARGUMENT; c->kd_fold = value; return 0; }
  if (option == BN254_OPT_KEY_DEDUP_FORCE_GENERIC) { c->kd_force_generic = value == 2 ? 2 : value != 0; return 0; }
  if (option == BN254_OPT_KEY_CACHE) { if (value < 0 || value > 1) return BN254_E_BAD_ARGUMENT; c->kd_cache = value; c->kd_cache_valid = false; return 0; }
  if (option == BN254_OPT_KEY_DEDUP_HASH_BITS) { if (value < 0 || value > 32) return BN254_E_BAD_ARGUMENT; c->kd_hash_bits = value; return 0; }
  if (option == BN254_OPT_AGGD_KEYED_ROUTE) { if (value < 0 || value > 3) return BN254_E_BAD_ARGUMENT; c->aggd_keyed_route = value; return 0; }
  if (option == BN254_OPT_AGG_RAND_MIN_PAIRS) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->agg_rand_min_pairs = value; return 0; }
  if (option == BN254_OPT_AGG_RAND_GROUP_PAIRS) { if (value < 1) return BN254_E_BAD_ARGUMENT; c->agg_rand_group_pairs = value; return 0; }
  if (option == BN254_OPT_BITMAP_TABLE_MAX_KEYS) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->bm_table_max_keys = value; return 0; }
  if (option == BN254_OPT_BITMAP_RAND_MIN_TUPLES) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->bmr_min_tuples = value; return 0; }
  if (option == BN254_OPT_BITMAP_RAND_MAX_KEYS) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->bmr_max_keys = value; return 0; }
  if (option == BN254_OPT_COLLECT_WAVE_MIN_SHARES) { if (value < 1) return BN254_E_BAD_ARGUMENT; c->collect_wave_min = value; return 0; }
  if (option == BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS) { if (value < 1) return BN254_E_BAD_ARGUMENT; c->pe_wave_min = value; return 0; }
  if (option == BN254_OPT_COLLECT_RAND_MIN_SHARES) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->collect_rand_min_shares = value; return 0; }
  if (option == BN254_OPT_COLLECT_RAND_MIN_PER_KEY) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->collect_rand_min_per_key = value; return 0; }
  if (option == BN254_OPT_THRESHOLD_OPT_MIN_SHARES) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->th_opt_min_shares = value; return 0; }
  if (option == BN254_OPT_COLLECT_OPT_MIN_SHARES) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->collect_opt_min_shares = value; return 0; }
  if (option == BN254_OPT_MERGE_WAVE_MIN_PARTS) { if (value < 1) return BN254_E_BAD_ARGUMENT; c->merge_wave_min = value; return 0; }
  if (option == BN254_OPT_MERGE_OPT_MIN_PARTS) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->merge_opt_min_parts = value; return 0; }
  if (option == BN254_OPT_COLLECT_OPT_MIN_TUPLE_SHARES) { if (value < 0) return BN254_E_BAD_ARGUMENT; c->collect_opt_min_tuple_shares = value; return 0; }
  if (option == BN254_OPT_BITMAP_RAND_GROUP_TUPLES) { if (value < 1) return BN254_E_BAD_ARGUMENT; c->bmr_group_tuples = value; return 0; }
  if (option == BN254_OPT_BITMAP_ROUTE) { if (value < 0 || value > 2) return BN254_E_BAD_ARGUMENT; c->bm_route = value; return 0; }
  return BN254_E_BAD_ARGUMENT;
}
// clock probe (BN254_OPT_CLOCK_PROBE): the clock the chip ran the last Miller kernel [0], final exponentiation [1] and issue probe [2]
// at, in MHz = shader-clock cycles / constant-rate ticks x the constant rate, summed over the workgroups that reported; 0 = none did
int bn254_ctx_last_clocks(bn254_ctx* c, double sclk_mhz[3]) {
  if (!c || !sclk_mhz || !c->ws.clk) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  int wall_khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, c->device));
  const size_t words = (size_t)3 * BN_CLK_MAX_WG * 2;
  unsigned long long* h = (unsigned long long*)malloc(words * sizeof(unsigned long long));
  if (!h) return BN254_E_NO_MEMORY;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h, c->ws.clk, words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemset(c->ws.clk, 0, words * sizeof(unsigned long long));     // read AND cleared: the next reading covers the launches from here on
  if (e != hipSuccess) { free(h); return -(int)e; }
  for (int k = 0; k < 3; ++k) {
    double cyc = 0, wall = 0;
    for (size_t w = 0; w < BN_CLK_MAX_WG; ++w) {
      const unsigned long long a = h[((size_t)k * BN_CLK_MAX_WG + w) * 2], b = h[((size_t)k * BN_CLK_MAX_WG + w) * 2 + 1];
      if (b) { cyc += (double)a; wall += (double)b; }
    }
    sclk_mhz[k] = wall > 0 ? cyc / wall * (double)wall_khz * 1e-3 : 0.0;
  }
  free(h);
  return 0;
}
int bn254_ctx_last_kernel_ms(bn254_ctx* c, float ms[4]) {
  if (!c || !ms || !c->ev_valid) return BN254_E_BAD_ARGUMENT;
  if (c->ev_layout == EV_COLLECT) {                       // bn254_batch_collect_keyed_bitmap: its select-and-sum runs last and reports in ms[1]
    static const int from[4] = {1, 4, 2, 3}, to[4] = {2, 0, 3, 4};
    HIP_TRY(hipEventSynchronize(c->ev[0]));
    for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->ev[from[i]], c->ev[to[i]]));
    return 0;
  }
  HIP_TRY(hipEventSynchronize(c->ev[4]));
  for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
  // the host-pointer verify hashes FIRST (the messages cross PCIe first) and decodes second: keep the documented slots
  // (ms[0] decode, ms[1] hash-to-G1 — there including the transfer of the messages)
  if (c->ev_layout == EV_HASH_FIRST) { float t = ms[0]; ms[0] = ms[1]; ms[1] = t; }
  return 0;
}


}  // extern "C"
// final exponentiation of a verify-shaped batch in the layout of its routing-table row (bn254_ws.h: bn_route): lane pairs; small batches in
// the octet layout; the smallest on nine lane pairs per verify (bn254_nonet.hip; eighteen while one verify per wave still covers the batch) —
// fewer instructions per lane again.  Callers with a Miller kernel of their own (the keyed lane machine, aggd_device) pass route_for(c, n).fe.
int launch_final_exp_layout(bn254_ctx* c, hipStream_t s, size_t n, int use_hash, uint8_t* d_status, int fe) {
  switch (fe) {
    case BN_FE_NONET_WIDE: return bn254_nonet_final_exp(n, c->ws, use_hash, d_status, s, 1);
    case BN_FE_NONET: return bn254_nonet_final_exp(n, c->ws, use_hash, d_status, s, 0);
    case BN_FE_OCTET: return bn254_trio_final_exp(n, c->ws, use_hash, d_status, s);
    default: return bn254_pair_final_exp(n, c->ws, use_hash, d_status, nullptr, nullptr, s);
  }
}
// Miller loop + final exponentiation of a verify-shaped batch on lane pairs, or — for batches that cannot fill the chip — in the octet layout
// (three lane pairs share the Fq6 products of every Fq12 operation: fewer instructions per lane, which is what latency is made of when a wave
// has its SIMD to itself).  Same status bytes either way.  BN254_OPT_PAIR_LANES = 0: one lane per item, the fused two-pair loop (A/B layout).
int launch_verify_miller_fe(bn254_ctx* c, hipStream_t s, size_t n, int pairs, int use_hash, uint8_t* d_status, bool mark) {
  if (!c->pair_lanes) {
    const unsigned g = grid_for(n);
    if (pairs == BN_PAIRS_CHECK_PKS) k_miller_cpk<<<g, BN_WAVE, 0, s>>>(n, c->ws);
    else k_miller_verify<<<g, BN_WAVE, 0, s>>>(n, c->ws, nullptr, nullptr);
    if (mark) PROF_MARK(3);
    k_final_exp<<<g, BN_WAVE, 0, s>>>(n, 1, 1, 1, c->ws, use_hash, nullptr, d_status, 0, 0, nullptr, nullptr);
    return 0;
  }
  const BnRoute r = route_for(c, n);
  int rc;
  switch (r.miller) {
    case BN_ML_LANE_MACHINE: rc = bn254_lm_miller_verify(n, c->ws, s, pairs); break;
    case BN_ML_WAVE_ROLES:         // BN254_OPT_TRIO_WAVE_ROLES (developer knob): eight waves (default), four, or the lane groups of one wave
      rc = c->trio_wave_roles == 2 ? bn254_w8_miller_verify(n, c->ws, s, pairs)
           : c->trio_wave_roles ? bn254_quad_miller_verify(n, c->ws, s, pairs) : bn254_trio_miller_verify(n, c->ws, s, pairs);
      break;
    default: rc = bn254_pair_miller_verify(n, c->ws, nullptr, nullptr, s, pairs); break;
  }
  if (rc) return rc;
  if (mark) PROF_MARK(3);
  return launch_final_exp_layout(c, s, n, use_hash, d_status, r.fe);
}

extern "C" {
// the end of every verify (device and host-pointer): decode and hash have filled the P1 / P2 / Q planes — Miller loop, final exponentiation,
// the last profiling event.  kd: the key-dedup buffers when bn254_kd_enqueue runs beside decode and hash on c->kd_stream (joined by
// c->kd_join), else null; split: BN254_OPT_SPLIT_MILLER's layout; hash_first: the order of the intervals (bn254_ctx_last_kernel_ms)
static int verify_tail(bn254_ctx* c, hipStream_t s, size_t n, uint8_t* d_status, bool split, const KeyDedup* kd, int hash_first) {
  int rc;
  if (kd) {
    // both Miller kernels are enqueued; each reads its item count from the device-side decision (k_kd_decide) and one of them returns at
    // once.  The wait for the builder counts in the Miller stage.
    HIP_TRY(hipStreamWaitEvent(s, c->kd_join, 0));
    const KeyTable kt = {kd->lines, kd->st, kd->inf, kd->max_keys};
    if (c->kd_fold == 2) rc = bn254_pair_miller_verify_keyed_unit(n, c->ws, kd->key_idx, kt, s, 0, nullptr, kd->ctl + KD_CTL_KEYED_N);
    else if (c->kd_fold) rc = bn254_pair_miller_verify_keyed_fold(n, c->ws, kd->key_idx, kt, kd->fold, s, 0, nullptr, kd->ctl + KD_CTL_KEYED_N);
    else rc = bn254_pair_miller_verify_keyed(n, c->ws, kd->key_idx, kt, s, 0, nullptr, kd->ctl + KD_CTL_KEYED_N);
    if (rc) return rc;
    if ((rc = bn254_pair_miller_verify(n, c->ws, nullptr, kd->ctl + KD_CTL_GENERIC_N, s))) return rc;
    PROF_MARK(3);
    if ((rc = bn254_pair_final_exp(n, c->ws, 1, d_status, nullptr, nullptr, s))) return rc;
    HIP_TRY(hipEventRecord(c->kd_done, s));          // the next call of this route waits for it, whatever its stream (bn254_batch_verify_device)
  } else if (split) {
    const unsigned g = grid_for(n);
    k_miller_verify_split<<<2 * g, BN_WAVE, 0, s>>>(n, c->ws.stride / 2, g, c->ws);
    PROF_MARK(3);
    k_final_exp<<<g, BN_WAVE, 0, s>>>(n, 2, 1, c->ws.stride / 2, c->ws, 1, nullptr, d_status, 0, 0, nullptr, nullptr);
  } else if ((rc = launch_verify_miller_fe(c, s, n, BN_PAIRS_VERIFY, 1, d_status, true))) return rc;
  PROF_MARK(4);
  prof_done(c, hash_first ? EV_HASH_FIRST : EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}
// decode kernels have filled the P1 / Q planes and BY_ST_DECODE: hash, then the verify's tail
static int verify_after_decode(bn254_ctx* c, hipStream_t s, const uint8_t* d_msgs, const uint64_t* d_off, size_t n, uint8_t* d_status, bool split,
                               const KeyDedup* kd = nullptr) {
  PROF_MARK(1);
  if (const int rc = launch_hash_rounds(c, s, d_msgs, d_off, n, PL_P2X, BY_P2_INF, nullptr)) return rc;
  PROF_MARK(2);
  return verify_tail(c, s, n, d_status, split, kd, 0);
}

int bn254_batch_verify_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, const uint8_t* d_pks,
                              size_t n, uint32_t flags, uint8_t* d_status, void* stream) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || g1c_flag(flags) || (n && (!d_msgs || !d_off || !d_sigs || !d_pks || !d_status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_sigs) || misaligned(d_pks) || ((uintptr_t)d_off & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  // default: verify on lane pairs (bn254_pair.hip).  BN254_OPT_PAIR_LANES = 0: one lane per verify, fused 2-pair
  // loop; BN254_OPT_SPLIT_MILLER additionally runs one pairing per lane (two waves per verify) — both kept for A/B
  // runs, see profiles/r01_c_ab_occupancy.log and DESIGN.md section 4
  bool split = c->split_miller && n <= BN_SPLIT_MAX_N;
  // key dedup (bn254_keydedup.hip): batches on the lane-pair Miller kernel look for repeated keys and take the keyed loop when they pay off
  bool key_dedup = c->key_dedup && c->kd_max_keys > 0 && c->pair_lanes && !split && n <= 0xFFFFFFFFu &&
                         route_for(c, n).miller == BN_ML_LANE_PAIRS && route_for(c, n).fe == BN_FE_LANE_PAIRS;
  if (const size_t chunk = ws_chunk_for(c, n, split ? 2 : 1, key_dedup))
    return verify_device_sliced(n, chunk, [&](size_t lo, size_t len) {
      return bn254_batch_verify_device(c, d_msgs, d_off + lo, d_sigs + 64 * lo, d_pks + 128 * lo, len, flags, d_status + lo, stream);
    });
  int rc = ws_reserve(c, split ? 2 * n : n);
  if (rc) return rc;
  KeyDedup kd;
  if (key_dedup) {
    rc = kd_reserve(c, n, kd);
    if (rc == KD_NO_ROOM) key_dedup = false;
    else if (rc) return rc;
    rc = 0;
  }
  c->kd_last_run = key_dedup;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  PROF_MARK(0);
  if (key_dedup) {                                   // forked behind everything the caller's stream holds so far: d_pks is readable
    // The key cache outlives the call: its rows are written on kd_stream and read by this call's Miller kernel and by the next call's match
    // pass, and the dedup buffers beside it are rewritten by every call.  The next call may come on ANOTHER caller stream with no host sync in
    // between, so the context orders it itself: this call — its side-stream work through kd_fork — starts behind kd_done, recorded at the
    // end of the previous call of this route (never recorded yet: no wait).
    HIP_TRY(hipStreamWaitEvent(s, c->kd_done, 0));
    // a cached row depends on the key's bytes and on what the builder ran under: the decode flags, the hash seam of the index and the row
    // capacity.  When one of them differs from the last call's (or the buffers moved, or the option was set) the cache starts empty.
    const bool cache_reset = !c->kd_cache || !c->kd_cache_valid || c->kd_cache_flags != flags || c->kd_cache_max_keys != c->kd_max_keys ||
                             c->kd_cache_hash_bits != c->kd_hash_bits;
    c->kd_cache_valid = false;                       // until the call's dedup work is enqueued: a launch that fails leaves the cache to be emptied
    HIP_TRY(hipEventRecord(c->kd_fork, s));
    HIP_TRY(hipStreamWaitEvent(c->kd_stream, c->kd_fork, 0));
    if ((rc = bn254_kd_enqueue(d_pks, n, flags, kd, c->kd_force_generic, cache_reset, c->kd_cache, c->kd_stream))) return rc;
    HIP_TRY(hipEventRecord(c->kd_join, c->kd_stream));
    c->kd_cache_valid = c->kd_cache != 0;
    c->kd_cache_flags = flags; c->kd_cache_max_keys = c->kd_max_keys; c->kd_cache_hash_bits = c->kd_hash_bits;
  }
  k_decode_g1<<<grid_for(n), BN_WAVE, 0, s>>>(d_sigs, n, flags, c->ws, PL_P1X, BY_P1_INF, 0);
  if ((rc = launch_decode_g2(c, s, d_pks, n, flags, 1))) return rc;
  return verify_after_decode(c, s, d_msgs, d_off, n, d_status, split, key_dedup ? &kd : nullptr);
}

// the same from the COMPRESSED encodings callers store (serde, /root/reference/src/serde.rs:39, :54):
// signatures 33 B (src/utils.rs:84-104), public keys 65 B (src/utils.rs:130-158, subgroup-checked on decode)
int bn254_batch_verify_compressed_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs33,
                                         const uint8_t* d_pks65, size_t n, uint8_t* d_status, void* stream) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!d_msgs || !d_off || !d_sigs33 || !d_pks65 || !d_status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if ((uintptr_t)d_off & 7u) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  if (const size_t chunk = ws_chunk_for(c, n))
    return verify_device_sliced(n, chunk, [&](size_t lo, size_t len) {
      return bn254_batch_verify_compressed_device(c, d_msgs, d_off + lo, d_sigs33 + 33 * lo, d_pks65 + 65 * lo, len, d_status + lo, stream);
    });
  int rc = ws_reserve(c, n);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  PROF_MARK(0);
  k_decompress_g1_ws<<<grid_for(n), BN_WAVE, 0, s>>>(d_sigs33, n, c->ws);
  if (route_lane_machine_helpers(c, n)) {
    // the smallest batches: the subgroup test of the decompressed keys with its ladder in the lane machine's level tables
    if ((rc = bn254_pair_decompress_g2(d_pks65, n, c->ws, s, 1))) return rc;
    if ((rc = bn254_lm_g2_subgroup(n, c->ws, s, ST_NOT_MEMBER))) return rc;
  } else if (c->pair_lanes) { if ((rc = bn254_pair_decompress_g2(d_pks65, n, c->ws, s))) return rc; }
  else k_decompress_g2_ws<<<grid_for(n), BN_WAVE, 0, s>>>(d_pks65, n, c->ws);
  return verify_after_decode(c, s, d_msgs, d_off, n, d_status, false);
}
// An oversized host-pointer verify (bn254_batch_verify, _compressed): slices through the same entry point, each with its offsets rebased to
// its own first message byte
static int verify_host_sliced(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, const uint8_t* pks, size_t n,
                              uint32_t flags, uint8_t* status, size_t chunk, bool compressed) {
  uint64_t* tmp = (uint64_t*)malloc((chunk + 1) * sizeof(uint64_t));
  if (!tmp) return BN254_E_NO_MEMORY;
  const size_t sig_sz = compressed ? 33 : 64, pk_sz = compressed ? 65 : 128;
  int rc = 0;
  for (size_t lo = 0; lo < n && !rc; lo += chunk) {
    const size_t len = n - lo < chunk ? n - lo : chunk;
    for (size_t i = 0; i <= len; ++i) tmp[i] = off[lo + i] - off[lo];
    const uint8_t* m = msgs ? msgs + off[lo] : nullptr;
    rc = compressed ? bn254_batch_verify_compressed(c, m, tmp, sigs + sig_sz * lo, pks + pk_sz * lo, len, status + lo)
                    : bn254_batch_verify(c, m, tmp, sigs + sig_sz * lo, pks + pk_sz * lo, len, flags, status + lo);
  }
  free(tmp);
  return rc;
}
int bn254_batch_verify_compressed(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs33, const uint8_t* pks65, size_t n,
                                  uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!off || !sigs33 || !pks65 || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, off, n)) return BN254_E_BAD_ARGUMENT;
  if (const size_t chunk = ws_chunk_for(c, n)) return verify_host_sliced(c, msgs, off, sigs33, pks65, n, 0, status, chunk, true);
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)off[n]), *d_off = st.in(1, off, (n + 1) * sizeof(uint64_t));
  const uint8_t *d_sigs = st.in(2, sigs33, n * 33), *d_pks = st.in(3, pks65, n * 65);
  uint8_t* d_status = st.out(4, n, status);
  if (st.ok()) st.rc = bn254_batch_verify_compressed_device(c, d_msgs, (const uint64_t*)d_off, d_sigs, d_pks, n, d_status, nullptr);
  return st.finish();
}

// Pinned staging (BN254_OPT_PINNED_STAGING = T > 0): the caller's buffers are pageable, and a hipMemcpyAsync from pageable memory is
// staged by the runtime on the calling thread.  With the option the bytes go through the context's own pinned buffer instead: T
// threads (the caller's + T - 1 helpers, started per call) each copy a contiguous share of a buffer into it in 1 MB pieces and
// enqueue the DMA of every piece as soon as it is in place, so page copies and DMA overlap and the DMA runs at the link's rate.
static int pin_reserve(bn254_ctx* c, size_t bytes) {
  if (bytes <= c->pin_cap) return 0;
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }
  if (c->pin) { HIP_TRY(hipHostFree(c->pin)); c->pin = nullptr; c->pin_cap = 0; }
  const size_t cap = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  HIP_TRY(hipHostMalloc((void**)&c->pin, cap, hipHostMallocDefault));
  c->pin_cap = cap;
  return 0;
}
static int pinned_copy_in(bn254_ctx* c, uint8_t* d_dst, uint8_t* pin, const uint8_t* src, size_t bytes, hipStream_t stream, int threads) {
  if (!bytes) return 0;
  const size_t piece = (size_t)1 << 20;
  if (threads > 16) threads = 16;
  if (threads > 1 && bytes < 4 * piece) threads = 1;
  int rcs[16] = {0};
  auto work = [&](int t, int n_threads) {
    if (t && hipSetDevice(c->device) != hipSuccess) { rcs[t] = -1; return; }
    const size_t share = ((bytes + n_threads - 1) / n_threads + 255) & ~(size_t)255, lo = (size_t)t * share, hi = lo + share < bytes ? lo + share : bytes;
    for (size_t o = lo; o < hi; o += piece) {
      const size_t len = o + piece < hi ? piece : hi - o;
      memcpy(pin + o, src + o, len);
      const hipError_t e = hipMemcpyAsync(d_dst + o, pin + o, len, hipMemcpyHostToDevice, stream);
      if (e != hipSuccess) { rcs[t] = -(int)e; return; }
    }
  };
  // helper threads: nothing may unwind through the C ABI — if a thread cannot be created the caller's thread copies everything itself
  std::thread helpers[15];
  int started = 0;
  bool fallback = false;
  try {
    for (int t = 1; t < threads; ++t) { helpers[started] = std::thread(work, t, threads); ++started; }
  } catch (...) {
    fallback = true;
  }
  if (!fallback) work(0, threads);
  for (int t = 0; t < started; ++t) helpers[t].join();
  if (fallback) {                                   // the shares of the helpers that did start are done (and harmlessly redone here)
    for (int t = 0; t < 16; ++t) rcs[t] = 0;
    work(0, 1);
  }
  for (int t = 0; t < 16; ++t) if (rcs[t]) return rcs[t];
  return 0;
}
static int verify_host_overlapped(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, const uint8_t* pks, size_t n,
                                  uint32_t flags, uint8_t* status) {
  const size_t msg_bytes = (size_t)off[n];
  int rc;
  if ((rc = ws_reserve(c, n))) return rc;
  HostStaging st(c);               // the copies below go on two streams by hand; every return waits for both
  const size_t need[4] = {msg_bytes ? msg_bytes : 1, (n + 1) * sizeof(uint64_t), n * 64, n * 128};
  for (int slot = 0; slot < 4; ++slot) st.out(slot, need[slot]);
  st.out(4, n, status);
  if (!st.ok()) return st.rc;
  hipStream_t s = c->stream;
  const bool pinned = c->pinned_staging > 0 && n >= PINNED_STAGING_MIN_N;
  auto up = [](size_t x) { return (x + 4095) & ~(size_t)4095; };
  const size_t o_off = up(msg_bytes), o_sig = o_off + up((n + 1) * sizeof(uint64_t)), o_pk = o_sig + up(n * 64), pin_bytes = o_pk + up(n * 128);
  if (pinned && (rc = pin_reserve(c, pin_bytes))) return rc;
  PROF_MARK(0);
  if (pinned) {
    if ((rc = pinned_copy_in(c, c->stage[0], c->pin, msgs, msg_bytes, s, c->pinned_staging))) return rc;
    if ((rc = pinned_copy_in(c, c->stage[1], c->pin + o_off, (const uint8_t*)off, (n + 1) * sizeof(uint64_t), s, 1))) return rc;
  } else {
    if (msg_bytes) HIP_TRY(hipMemcpyAsync(c->stage[0], msgs, msg_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->stage[1], off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  }
  if ((rc = launch_hash_rounds(c, s, c->stage[0], (const uint64_t*)c->stage[1], n, PL_P2X, BY_P2_INF, nullptr))) return rc;
  if (pinned) {
    if ((rc = pinned_copy_in(c, c->stage[2], c->pin + o_sig, sigs, n * 64, c->copy_stream, c->pinned_staging))) return rc;
    if ((rc = pinned_copy_in(c, c->stage[3], c->pin + o_pk, pks, n * 128, c->copy_stream, c->pinned_staging))) return rc;
  } else {
    HIP_TRY(hipMemcpyAsync(c->stage[2], sigs, n * 64, hipMemcpyHostToDevice, c->copy_stream));
    HIP_TRY(hipMemcpyAsync(c->stage[3], pks, n * 128, hipMemcpyHostToDevice, c->copy_stream));
  }
  HIP_TRY(hipEventRecord(c->copy_done, c->copy_stream));
  HIP_TRY(hipStreamWaitEvent(s, c->copy_done, 0));
  PROF_MARK(1);
  k_decode_g1<<<grid_for(n), BN_WAVE, 0, s>>>(c->stage[2], n, flags, c->ws, PL_P1X, BY_P1_INF, 0);
  if ((rc = launch_decode_g2(c, s, c->stage[3], n, flags, 1))) return rc;
  PROF_MARK(2);
  if ((rc = verify_tail(c, s, n, c->stage[4], false, nullptr, 1))) return rc;   // intervals: transfer + hash, decode, Miller, final exp.
  return st.finish();
}

// Host-buffer entry point.  The hash-to-G1 rounds need only the messages, so those cross PCIe first and the hash
// kernels start at once; signatures and public keys (5/6 of the bytes) follow on a second stream while the hash runs,
// and the decode kernels wait for them on an event.  What is left exposed of the transfer is the message copy and the
// status bytes coming back.
int bn254_batch_verify(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, const uint8_t* pks, size_t n,
                       uint32_t flags, uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || g1c_flag(flags) || (n && (!off || !sigs || !pks || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, off, n)) return BN254_E_BAD_ARGUMENT;
  if (c->split_miller && n <= BN_SPLIT_MAX_N) {      // A/B layout: plain staging, then the device entry point
    HostStaging st(c);
    const uint8_t *d_msgs = st.in(0, msgs, (size_t)off[n]), *d_off = st.in(1, off, (n + 1) * sizeof(uint64_t));
    const uint8_t *d_sigs = st.in(2, sigs, n * 64), *d_pks = st.in(3, pks, n * 128);
    uint8_t* d_status = st.out(4, n, status);
    if (st.ok()) st.rc = bn254_batch_verify_device(c, d_msgs, (const uint64_t*)d_off, d_sigs, d_pks, n, flags, d_status, nullptr);
    return st.finish();
  }
  if (const size_t chunk = ws_chunk_for(c, n)) return verify_host_sliced(c, msgs, off, sigs, pks, n, flags, status, chunk, false);
  return verify_host_overlapped(c, msgs, off, sigs, pks, n, flags, status);
}

int bn254_batch_hash_to_g1_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, size_t n, uint8_t* d_points, uint8_t* d_status,
                                  uint8_t* d_tries, void* stream) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!d_msgs || !d_off || !d_points || !d_status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_points) || ((uintptr_t)d_off & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  int rc = ws_reserve(c, n);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  unsigned g = grid_for(n);
  PROF_MARK(0);                                        // ms[0] = the filter rounds (init / round / resolve), ms[1] = k_hash_finish (the square roots),
  if ((rc = launch_hash_rounds(c, s, d_msgs, d_off, n, PL_P1X, BY_P1_INF, d_tries, 1))) return rc;     // ms[2] = encoding the points, ms[3] = 0
  PROF_MARK(2);
  k_encode_g1<<<g, BN_WAVE, 0, s>>>(n, c->ws, PL_P1X, BY_P1_INF, d_points, d_status);
  PROF_MARK(3);
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_batch_hash_to_g1(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, size_t n, uint8_t* points, uint8_t* status, uint8_t* tries) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!off || !points || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, off, n)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)off[n]), *d_off = st.in(1, off, (n + 1) * sizeof(uint64_t));
  uint8_t *d_points = st.out(2, n * 64, points), *d_status = st.out(3, n, status), *d_tries = st.out(4, n, tries);
  if (st.ok()) st.rc = bn254_batch_hash_to_g1_device(c, d_msgs, (const uint64_t*)d_off, n, d_points, d_status, d_tries, nullptr);
  return st.finish();
}

// shared by pairing / pairing_check: mode 0 = reduced Gt + status, 1 = raw Miller value (debug)
static int pairing_device(bn254_ctx* c, const uint8_t* d_g1, const uint8_t* d_g2, size_t n, size_t k, uint32_t flags, uint8_t* d_gt,
                          uint8_t* d_status, void* stream, int raw_only) {
  if (!c || k == 0 || g1c_flag(flags) || (n && (!d_g1 || !d_g2))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_g1) || misaligned(d_g2) || (d_gt && misaligned(d_gt))) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  size_t lanes = n * k;
  int rc = ws_reserve(c, lanes);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  PROF_MARK(0);
  k_decode_g1<<<grid_for(lanes), BN_WAVE, 0, s>>>(d_g1, lanes, flags, c->ws, PL_P1X, BY_P1_INF, 0);
  if ((rc = launch_decode_g2(c, s, d_g2, lanes, flags, 1))) return rc;
  PROF_MARK(1);
  PROF_MARK(2);                                      // no hash in a pairing: ms[1] = 0
  if (!raw_only && route_lane_machine_helpers(c, lanes) && route_for(c, n).fe == BN_FE_NONET_WIDE) {
    // a batch that cannot fill the chip: the small-batch kernels of a verify — the lane machine with the fixed
    // pair skipped, the final exponentiation (exact program, Gt bytes) on eighteen lane pairs per item: 5.7 -> 1.3 ms for one pairing
    if ((rc = bn254_lm_miller_verify(lanes, c->ws, s, 2))) return rc;
    PROF_MARK(3);
    if ((rc = bn254_nonet_final_exp_product(n, k, c->ws, d_gt, d_status, s))) return rc;
  } else if (c->pair_lanes) {
    if ((rc = bn254_pair_miller_var(lanes, c->ws, s))) return rc;
    PROF_MARK(3);
    if ((rc = bn254_pair_final_exp_product(n, k, c->ws, d_gt, d_status, raw_only, s))) return rc;
  } else {
    k_miller_var<<<grid_for(lanes), BN_WAVE, 0, s>>>(lanes, c->ws);
    PROF_MARK(3);
    k_final_exp<<<grid_for(n), BN_WAVE, 0, s>>>(n, k, k, 1, c->ws, 0, d_gt, d_status, raw_only, 0, nullptr, nullptr);
  }
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}
int bn254_batch_pairing_device(bn254_ctx* c, const uint8_t* d_g1, const uint8_t* d_g2, size_t n, size_t k, uint32_t flags, uint8_t* d_gt,
                               uint8_t* d_status, void* stream) {
  return pairing_device(c, d_g1, d_g2, n, k, flags, d_gt, d_status, stream, 0);
}
static int pairing_host(bn254_ctx* c, const uint8_t* g1, const uint8_t* g2, size_t n, size_t k, uint32_t flags, uint8_t* gt, uint8_t* status,
                        int raw_only) {
  if (!c || k == 0 || g1c_flag(flags) || (n && (!g1 || !g2))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t *d_g1 = st.in(0, g1, n * k * 64), *d_g2 = st.in(1, g2, n * k * 128);
  uint8_t *d_gt = st.out(2, n * 384, gt), *d_status = st.out(3, n, status);
  if (st.ok()) st.rc = pairing_device(c, d_g1, d_g2, n, k, flags, gt ? d_gt : nullptr, d_status, nullptr, raw_only);
  return st.finish();
}
int bn254_batch_pairing_check(bn254_ctx* c, const uint8_t* g1, const uint8_t* g2, size_t n, size_t k, uint32_t flags, uint8_t* status) {
  if (!status && n) return BN254_E_BAD_ARGUMENT;
  return pairing_host(c, g1, g2, n, k, flags, nullptr, status, 0);
}
int bn254_batch_pairing(bn254_ctx* c, const uint8_t* g1, const uint8_t* g2, size_t n, size_t k, uint32_t flags, uint8_t* gt, uint8_t* status) {
  if (!gt && n) return BN254_E_BAD_ARGUMENT;
  return pairing_host(c, g1, g2, n, k, flags, gt, status, 0);
}
int bn254_debug_miller_loop(bn254_ctx* c, const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* f) {
  if (!f && n) return BN254_E_BAD_ARGUMENT;
  return pairing_host(c, g1, g2, n, 1, 0, f, nullptr, 1);
}

int bn254_batch_check_public_keys(bn254_ctx* c, const uint8_t* pk_g2, const uint8_t* pk_g1, size_t n, uint32_t flags, uint8_t* status) {
  if (!c || g1c_flag(flags) || (n && (!pk_g2 || !pk_g1 || !status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = ws_reserve(c, n))) return rc;
  HostStaging st(c);
  const uint8_t *d_g2 = st.in(0, pk_g2, n * 128), *d_g1 = st.in(1, pk_g1, n * 64);
  uint8_t* d_status = st.out(2, n, status);
  if (!st.ok()) return st.rc;
  hipStream_t s = c->stream;
  if ((rc = launch_decode_g2(c, s, d_g2, n, flags, 0))) return rc;       // ecdsa.rs:82: pk_g2 first
  k_decode_g1<<<grid_for(n), BN_WAVE, 0, s>>>(d_g1, n, flags, c->ws, PL_P1X, BY_P1_INF, 1);
  if ((rc = launch_verify_miller_fe(c, s, n, BN_PAIRS_CHECK_PKS, 0, d_status, false))) return rc;
  HIP_TRY(hipGetLastError());
  return st.finish();
}

}  // extern "C"
