// Translation unit of libbn254hip.so: what the signer-bitmap calls return besides a status byte (include/bn254_hip.h:
// bn254_batch_aggregate_keys_bitmap[_device], bn254_batch_verify_keyed_bitmap_export[_device], bn254_ctx_set_key_weights,
// bn254_batch_bitmap_weights[_device]) — the emit, settle and weight kernels and the host side of the entry points.  The per-item bodies
// are bn254_bitmap_out.h, shared with the CPU suite's host compilation; the sums themselves are the bitmap verify's (bn254_bitmap.hip:
// bm_prepare, launch_bitmap_sum), called and not altered.
// Per-tuple semantics: the aggregate key is `Add for PublicKey` over the set keys (the reference's src/types.rs:126-132); H(m) and the key
// are what the reference's precompile formatters are built from (src/utils.rs:197-239).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/bn254_hip.h"
#include "bn254_hash.h"
#include "bn254_io.h"
#include "bn254_pairing.h"
#include "bn254_bitmap.h"
#include "bn254_bitmap_out.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"

// The emit: one entry per lane.  The Q planes are the same words whichever layout summed them (k_bm_sum: ws_store_g2; k_bm_sum_pair: each
// role its half of the same planes), so ONE kernel reads them for both.  keys / hashes / status_out: each may be null.
KERNEL_SMALL void k_bmo_emit(size_t n, Ws ws, uint8_t* keys, uint8_t* hashes, uint8_t* status_out) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = ws_byte(ws, BY_ST_DECODE, i);
  if (keys)
    bmo_emit_key(keys + 128 * i, ws_load_fp(ws, PL_QX0, i), ws_load_fp(ws, PL_QX1, i), ws_load_fp(ws, PL_QY0, i), ws_load_fp(ws, PL_QY1, i),
                 ws_byte(ws, BY_Q_INF, i) != 0, st);
  if (hashes)
    bmo_emit_hash(hashes + 64 * i, ws_load_fp(ws, PL_P2X, i), ws_load_fp(ws, PL_P2Y, i), ws_byte(ws, BY_P2_INF, i) != 0,
                  st != ST_OK ? st : ws_byte(ws, BY_ST_HASH, i));
  if (status_out) status_out[i] = st;
}
// behind the verify: the outputs of the tuples that did not pass rules 1-3
KERNEL_SMALL void k_bmo_settle(size_t n, const uint8_t* status, uint8_t* hashes, uint8_t* keys) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  bmo_settle_item(status[i], hashes ? hashes + 64 * i : nullptr, keys ? keys + 128 * i : nullptr);
}
// the weight tables: one entry per lane
KERNEL_SMALL void k_bmw_build(const uint64_t* weights, uint32_t n_keys, size_t entries, uint64_t* tab) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (j < entries) tab[j] = bmw_subset_entry(weights, n_keys, (uint32_t)(j >> 8), (uint32_t)(j & 255u));
}
// the weight of a row: one tuple per lane, the tables read where they lie in device memory (2 KB per 8 keys: 64 KB at 256 keys, 1 MB at
// 4 096 — resident in the caches for every set this library tabulates).  ONE path for every key count and batch size: no boundary, no option.
KERNEL_SMALL void k_bmw_sum(const uint32_t* bits, size_t bm_words, size_t n, BmKeys K, const uint64_t* tab, uint64_t* weight, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  uint64_t w;
  uint8_t st;
  bmw_item(bits + i * bm_words, bm_words, K, tab, w, st);
  weight[i] = w;
  status[i] = st;
}

static inline uint8_t* ws_byte_plane(const bn254_ctx* c, int plane) { return c->ws.bytes + (size_t)plane * c->ws.stride; }
static int launch_bmo_emit(bn254_ctx* c, hipStream_t s, size_t n, uint8_t* d_keys, uint8_t* d_hashes, uint8_t* d_status) {
  k_bmo_emit<<<grid_for(n), BN_WAVE, 0, s>>>(n, c->ws, d_keys, d_hashes, d_status);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

// ---- A: the aggregate keys of bitmaps ------------------------------------------------------------------------------------------------------
int bn254_batch_aggregate_keys_bitmap_device(bn254_ctx* c, const uint32_t* d_bits, size_t bm_words, size_t n, uint32_t flags, uint8_t* d_keys,
                                             uint8_t* d_status, void* stream) {
  if (!c || flags != 0 || (n && (!d_keys || !d_status || (bm_words && !d_bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_bits) || misaligned(d_keys)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  if (const size_t chunk = ws_chunk_for(c, n))         // tuples are independent: a slice is the same arrays further in
    return verify_device_sliced(n, chunk, [&](size_t lo, size_t len) {
      return bn254_batch_aggregate_keys_bitmap_device(c, d_bits ? d_bits + lo * bm_words : nullptr, bm_words, len, flags, d_keys + 128 * lo, d_status + lo, stream);
    });
  int rc = ws_reserve(c, n);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  const bool tables = bm_wants_tables(c);
  if ((rc = bm_prepare(c, s, tables))) return rc;
  HIP_TRY(hipMemsetAsync(ws_byte_plane(c, BY_ST_DECODE), 0, n, s));   // the sum kernels write rule 2 BEHIND the entry's decode status: there is none here
  if ((rc = launch_bitmap_sum(c, s, d_bits, bm_words, n, tables))) return rc;
  return launch_bmo_emit(c, s, n, d_keys, nullptr, d_status);
}

int bn254_batch_aggregate_keys_bitmap(bn254_ctx* c, const uint32_t* bits, size_t bm_words, size_t n, uint32_t flags, uint8_t* agg_keys, uint8_t* status) {
  if (!c || flags != 0 || (n && (!agg_keys || !status || (bm_words && !bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_bits = st.in(3, bits, n * bm_words * sizeof(uint32_t));
  uint8_t* d_status = st.out(4, n, status);
  uint8_t* d_keys = st.out(5, n * 128, agg_keys);
  if (st.ok()) st.rc = bn254_batch_aggregate_keys_bitmap_device(c, (const uint32_t*)d_bits, bm_words, n, flags, d_keys, d_status, nullptr);
  return st.finish();
}

// ---- B: the bitmap verify that returns what it computed ------------------------------------------------------------------------------------
int bn254_batch_verify_keyed_bitmap_export_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, const uint32_t* d_bits,
                                                  size_t bm_words, size_t n, uint32_t flags, uint8_t* d_status, uint8_t* d_hashes, uint8_t* d_keys,
                                                  void* stream) {
  if (g1c_flag(flags))                                  // compressed aggregates: staged once, in front of any slicing.  The overlay behind the call
    return g1c_call(c, d_sigs, n, n != 0, d_status, stream, [&](const uint8_t* d_sigs64) {   // turns a 6 into a 3: neither keeps its outputs
      return bn254_batch_verify_keyed_bitmap_export_device(c, d_msgs, d_off, d_sigs64, d_bits, bm_words, n, flags & ~BN254_FLAG_G1_COMPRESSED, d_status,
                                                           d_hashes, d_keys, stream);
    });
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!d_msgs || !d_off || !d_sigs || !d_status || (bm_words && !d_bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_sigs) || misaligned(d_bits) || ((uintptr_t)d_off & 7u) || misaligned(d_hashes) || misaligned(d_keys)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  if (const size_t chunk = ws_chunk_for(c, n))
    return verify_device_sliced(n, chunk, [&](size_t lo, size_t len) {
      return bn254_batch_verify_keyed_bitmap_export_device(c, d_msgs, d_off + lo, d_sigs + 64 * lo, d_bits ? d_bits + lo * bm_words : nullptr, bm_words, len,
                                                           flags, d_status + lo, d_hashes ? d_hashes + 64 * lo : nullptr, d_keys ? d_keys + 128 * lo : nullptr,
                                                           stream);
    });
  int rc = ws_reserve(c, n);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  const bool tables = bm_wants_tables(c);
  if ((rc = bm_prepare(c, s, tables))) return rc;
  PROF_MARK(0);                                        // the bitmap verify's intervals; the emit counts in ms[1], the settle in ms[3]
  if ((rc = launch_decode_g1(c, s, d_sigs, n, flags, PL_P1X, BY_P1_INF, 0))) return rc;
  if ((rc = launch_hash_rounds(c, s, d_msgs, d_off, n, PL_P2X, BY_P2_INF, nullptr))) return rc;
  PROF_MARK(1);
  if ((rc = launch_bitmap_sum(c, s, d_bits, bm_words, n, tables))) return rc;
  // into the caller's buffers NOW: nothing says the P2 and Q planes survive the Miller loop and the final exponentiation
  if ((d_hashes || d_keys) && (rc = launch_bmo_emit(c, s, n, d_keys, d_hashes, nullptr))) return rc;
  PROF_MARK(2);
  if ((rc = launch_verify_miller_fe(c, s, n, BN_PAIRS_VERIFY, 1, d_status, true))) return rc;
  if (d_hashes || d_keys) k_bmo_settle<<<grid_for(n), BN_WAVE, 0, s>>>(n, d_status, d_hashes, d_keys);
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}

int bn254_batch_verify_keyed_bitmap_export(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, const uint32_t* bits, size_t bm_words,
                                           size_t n, uint32_t flags, uint8_t* status, uint8_t* hashes, uint8_t* agg_keys) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!off || !sigs || !status || (bm_words && !bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, off, n)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)off[n]), *d_off = st.in(1, off, (n + 1) * sizeof(uint64_t));
  const uint8_t *d_sigs = st.in(2, sigs, n * g1_item_bytes(flags)), *d_bits = st.in(3, bits, n * bm_words * sizeof(uint32_t));
  uint8_t* d_status = st.out(4, n, status);
  uint8_t* d_hashes = hashes ? st.out(5, n * 64, hashes) : nullptr;
  uint8_t* d_keys = agg_keys ? st.out(6, n * 128, agg_keys) : nullptr;
  if (st.ok())
    st.rc = bn254_batch_verify_keyed_bitmap_export_device(c, d_msgs, (const uint64_t*)d_off, d_sigs, (const uint32_t*)d_bits, bm_words, n, flags, d_status,
                                                          d_hashes, d_keys, nullptr);
  return st.finish();
}

// ---- C: the voting weight of bitmaps -------------------------------------------------------------------------------------------------------
int bn254_ctx_set_key_weights(bn254_ctx* c, const uint64_t* weights, size_t n_keys) {
  if (!c) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  { int rc_ = ctx_quiesce(c); if (rc_) return rc_; }   // no weight call may still be reading the previous tables
  c->bw_set = false;
  if (!weights) return 0;
  if (n_keys != c->n_keys) return BN254_E_BAD_ARGUMENT;
  uint64_t total = 0;
  for (size_t j = 0; j < n_keys; ++j)
    if (__builtin_add_overflow(total, weights[j], &total)) return BN254_E_BAD_ARGUMENT;   // the total must stay below 2^64: then no subset sum wraps
  const size_t entries = ((n_keys + 7) / 8) * BMW_WINDOW_ENTRIES;
  if (const int rc = scratch_reserve(c, &c->bw_tab, &c->bw_tab_cap, entries * sizeof(uint64_t))) return rc;
  if (n_keys) {
    HostStaging st(c);
    const uint8_t* d_w = st.in(3, weights, n_keys * sizeof(uint64_t));
    if (!st.ok()) return st.rc;
    k_bmw_build<<<grid_for(entries), BN_WAVE, 0, c->stream>>>((const uint64_t*)d_w, (uint32_t)n_keys, entries, (uint64_t*)c->bw_tab);
    st.check(hipGetLastError());
    if (const int rc = st.finish()) return rc;
  }
  c->bw_set = true;
  return 0;
}

int bn254_batch_bitmap_weights_device(bn254_ctx* c, const uint32_t* d_bits, size_t bm_words, size_t n, uint64_t* d_weight, uint8_t* d_status, void* stream) {
  if (!c || !c->bw_set || (n && (!d_weight || !d_status || (bm_words && !d_bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_bits) || ((uintptr_t)d_weight & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  if (const int rc = bm_prepare(c, s, false)) return rc;   // rule 2 reads the bad-bit vector; the call takes no workspace, so there is nothing to slice
  const BmKeys K = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)c->n_keys};
  k_bmw_sum<<<grid_for(n), BN_WAVE, 0, s>>>(d_bits, bm_words, n, K, (const uint64_t*)c->bw_tab, d_weight, d_status);
  HIP_TRY(hipGetLastError());
  return 0;
}

int bn254_batch_bitmap_weights(bn254_ctx* c, const uint32_t* bits, size_t bm_words, size_t n, uint64_t* weight, uint8_t* status) {
  if (!c || !c->bw_set || (n && (!weight || !status || (bm_words && !bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_bits = st.in(3, bits, n * bm_words * sizeof(uint32_t));
  uint8_t* d_status = st.out(4, n, status);
  uint8_t* d_weight = st.out(5, n * sizeof(uint64_t), weight);
  if (st.ok()) st.rc = bn254_batch_bitmap_weights_device(c, (const uint32_t*)d_bits, bm_words, n, (uint64_t*)d_weight, d_status, nullptr);
  return st.finish();
}

}  // extern "C"
