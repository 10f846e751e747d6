// Translation unit of libbn254hip.so: same-message aggregates given as SIGNER BITMAPS over the registered keys (include/bn254_hip.h:
// bn254_batch_verify_keyed_bitmap[_device]) — the subset tables of the registered set and their builder, the one-lane form of the sum, and
// the host side of the two entry points.  The sum on lane pairs is bn254_bitmap_pair.hip; the walk, the builder's arithmetic and rule 2 are
// bn254_bitmap.h, shared with the CPU suite's host compilation.
// Per-tuple semantics: ECDSA::verify (/root/reference/src/ecdsa.rs:49-64) against the sum of the selected keys (`Add for PublicKey`,
// src/types.rs:126-132; the reference aggregates for one common message, src/lib.rs:34-38).
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

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"

// the bad-bit vector of the registered set: one word per lane
KERNEL_SMALL void k_bm_bad_words(const uint8_t* key_st, uint32_t n_keys, uint32_t n_words, uint32_t* bad) {
  const uint32_t w = blockIdx.x * BN_WAVE + threadIdx.x;
  if (w < n_words) bad[w] = bm_bad_word(key_st, n_keys, w);
}
// the subset tables: one entry per lane (entry = window * 256 + mask: up to 8 additions and one inversion); lanes past the end add identities
KERNEL void k_bm_build_tables(BmKeys K, size_t n_windows, BmTable T) {
  const size_t j = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = j < n_windows * 256;
  G2Affine a;
  bm_subset_entry(a, K, (uint32_t)((live ? j : 0) >> 8), (uint32_t)(j & 255u), live);
  if (!live) return;
  bm_store_entry(T, j, a);
  T.inf[j] = a.inf;
}
// the sum, one tuple per lane (contexts with pair lanes off): what k_aggregate is to k_aggregate_pair.  Same walk, same outputs as
// k_bm_sum_pair.  No early return: the additions vote across the wave.
KERNEL void k_bm_sum(const uint32_t* bits, size_t bm_words, size_t n, BmKeys K, const int32_t* rec, const uint8_t* rec_inf, Ws ws) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  const bool live = i < n;
  const uint32_t* row = bits + (live ? i : 0) * bm_words;
  G2Jac acc;
  if (rec) bm_sum_tables(acc, row, bm_words, live, K, rec, rec_inf);      // wave-uniform
  else bm_sum_keys(acc, row, bm_words, live, K);
  G2Affine pk;
  bm_sum_to_key(pk, acc);
  if (!live) return;
  const uint8_t prev = ws_byte(ws, BY_ST_DECODE, i);
  ws_store_g2(ws, i, pk);
  ws_byte(ws, BY_ST_DECODE, i) = prev != ST_OK ? prev : bm_rule2_status(row, bm_words, K);
}

// does this call read tables?  BN254_OPT_BITMAP_ROUTE forces either answer (tests); otherwise the size rule of BN254_OPT_BITMAP_TABLE_MAX_KEYS
bool bm_wants_tables(const bn254_ctx* c) {
  if (c->n_keys == 0 || c->bm_route == 2) return false;
  return c->bm_route == 1 || (c->bm_table_max_keys > 0 && c->n_keys <= (size_t)c->bm_table_max_keys);
}
// Built lazily, on the call's stream, by the first bitmap call after a registration: the bad-bit vector always, the subset tables when the
// call reads them.  The context carries one call in flight, so every later call — on this stream, or on another one after this call has
// finished — is ordered behind the build.
int bm_prepare(bn254_ctx* c, hipStream_t s, bool tables) {
  if (c->n_keys == 0) return 0;
  if (!c->bm_bad_valid) {
    const uint32_t n_words = (uint32_t)((c->n_keys + 31) / 32);
    if (const int rc = scratch_reserve(c, &c->bm_bad, &c->bm_bad_cap, (size_t)n_words * sizeof(uint32_t))) return rc;
    k_bm_bad_words<<<grid_for(n_words), BN_WAVE, 0, s>>>(c->key_st, (uint32_t)c->n_keys, n_words, (uint32_t*)c->bm_bad);
    HIP_TRY(hipGetLastError());
    c->bm_bad_valid = true;
  }
  if (tables && !c->bm_tab_valid) {
    const size_t n_windows = (c->n_keys + 7) / 8, entries = n_windows * 256;
    if (const int rc = scratch_reserve(c, &c->bm_tab, &c->bm_tab_cap, entries * (BM_REC_WORDS * sizeof(int32_t) + 1))) return rc;
    const BmKeys K = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)c->n_keys};
    const BmTable T = {(int32_t*)c->bm_tab, c->bm_tab + entries * BM_REC_WORDS * sizeof(int32_t)};
    k_bm_build_tables<<<grid_for(entries), BN_WAVE, 0, s>>>(K, n_windows, T);
    HIP_TRY(hipGetLastError());
    c->bm_tab_valid = true;
  }
  return 0;
}

// the aggregate keys of n tuples whose P1 / P2 planes and decode statuses are filled: row i of d_bits summed into the Q planes of entry i, rule 2
// behind the decode status (bn254_host.h) — from the subset tables when `tables` (bm_prepare has built them), on lane pairs or one lane per tuple
int launch_bitmap_sum(bn254_ctx* c, hipStream_t s, const uint32_t* d_bits, size_t bm_words, size_t n, bool tables) {
  const int32_t* rec = tables ? (const int32_t*)c->bm_tab : nullptr;
  const uint8_t* rec_inf = tables ? c->bm_tab + ((c->n_keys + 7) / 8) * 256 * BM_REC_WORDS * sizeof(int32_t) : nullptr;
  if (c->pair_lanes) {
    const BmKeysArg ka = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)c->n_keys};
    return bn254_pair_bitmap_sum(d_bits, bm_words, n, ka, rec, rec_inf, c->ws, s);
  }
  const BmKeys K = {c->key_xy, c->key_st, c->key_inf, (const uint32_t*)c->bm_bad, (uint32_t)c->n_keys};
  k_bm_sum<<<grid_for(n), BN_WAVE, 0, s>>>(d_bits, bm_words, n, K, rec, rec_inf, c->ws);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

int bn254_batch_verify_keyed_bitmap_device(bn254_ctx* c, const uint8_t* d_msgs, const uint64_t* d_off, const uint8_t* d_sigs, const uint32_t* d_bits,
                                           size_t bm_words, size_t n, uint32_t flags, uint8_t* d_status, void* stream) {
  if (g1c_flag(flags))                                  // compressed aggregates: staged once, in front of any slicing
    return g1c_call(c, d_sigs, n, n != 0, d_status, stream, [&](const uint8_t* d_sigs64) {
      return bn254_batch_verify_keyed_bitmap_device(c, d_msgs, d_off, d_sigs64, d_bits, bm_words, n, flags & ~BN254_FLAG_G1_COMPRESSED, d_status, stream);
    });
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!d_msgs || !d_off || !d_sigs || !d_status || (bm_words && !d_bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_sigs) || misaligned(d_bits) || ((uintptr_t)d_off & 7u)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  if (const size_t chunk = ws_chunk_for(c, n))         // tuples are independent: a slice is the same arrays further in
    return verify_device_sliced(n, chunk, [&](size_t lo, size_t len) {
      return bn254_batch_verify_keyed_bitmap_device(c, d_msgs, d_off + lo, d_sigs + 64 * lo, d_bits ? d_bits + lo * bm_words : nullptr, bm_words, len, flags,
                                                    d_status + lo, stream);
    });
  int rc = ws_reserve(c, n);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  const bool tables = bm_wants_tables(c);
  if ((rc = bm_prepare(c, s, tables))) return rc;      // the first call after a registration builds here, ahead of the timed intervals
  PROF_MARK(0);                                        // ms[0] = sigma's decode + hash-to-G1, ms[1] = the aggregate keys, ms[2] / ms[3] as a verify
  if ((rc = launch_decode_g1(c, s, d_sigs, n, flags, PL_P1X, BY_P1_INF, 0))) return rc;
  if ((rc = launch_hash_rounds(c, s, d_msgs, d_off, n, PL_P2X, BY_P2_INF, nullptr))) return rc;
  PROF_MARK(1);
  if ((rc = launch_bitmap_sum(c, s, d_bits, bm_words, n, tables))) return rc;
  PROF_MARK(2);
  // the tuples are verify-shaped now: the routing table serves small batches with the small-batch kernels, as after the aggregation kernel
  if ((rc = launch_verify_miller_fe(c, s, n, BN_PAIRS_VERIFY, 1, d_status, true))) return rc;
  PROF_MARK(4);
  prof_done(c, EV_DECODE_FIRST);
  HIP_TRY(hipGetLastError());
  return 0;
}

int bn254_batch_verify_keyed_bitmap(bn254_ctx* c, const uint8_t* msgs, const uint64_t* off, const uint8_t* sigs, const uint32_t* bits, size_t bm_words,
                                    size_t n, uint32_t flags, uint8_t* status) {
  MsgsLenScope msgs_len_scope(c);
  if (!c || (n && (!off || !sigs || !status || (bm_words && !bits))) || bm_words > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (!msgs_ok(msgs, off, n)) return BN254_E_BAD_ARGUMENT;
  HostStaging st(c);
  const uint8_t *d_msgs = st.in(0, msgs, (size_t)off[n]), *d_off = st.in(1, off, (n + 1) * sizeof(uint64_t));
  const uint8_t *d_sigs = st.in(2, sigs, n * g1_item_bytes(flags)), *d_bits = st.in(3, bits, n * bm_words * sizeof(uint32_t));
  uint8_t* d_status = st.out(4, n, status);
  if (st.ok())
    st.rc = bn254_batch_verify_keyed_bitmap_device(c, d_msgs, (const uint64_t*)d_off, d_sigs, (const uint32_t*)d_bits, bm_words, n, flags, d_status, nullptr);
  return st.finish();
}

}  // extern "C"
