// Translation unit of libbn254hip.so: proofs of possession (include/bn254_hip.h: bn254_batch_pop_prove[_device], bn254_batch_pop_verify[_device],
// bn254_ctx_register_keys_pop) — the remedy the reference names for rogue keys (the reference, src/lib.rs:34-38: every key holder proves
// possession "by signing a message").  The proof of a key is its holder's signature on BN254_POP_TAG || pk, so every pairing, hash and
// ladder here is an existing route: the verify (bn254_hip.hip), key derivation and sign (bn254_group.hip), and for a registration the keyed
// route on the key's own freshly built line table (bn254_rand.hip: launch_keyed_miller_fe, all three of its branches).  This unit's own
// kernels are the front end — the composer of the proof messages and the fold of two status arrays; their bodies are bn254_pop.h, shared
// with the CPU suite's host compilation.
// Per-item semantics: ECDSA::sign / ::verify (src/ecdsa.rs:26-35, :49-64) on the composed message; the hash is the
// project's one hash-to-G1 (src/hash.rs:29-63).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/bn254_hip.h"
#include "bn254_hash.h"
#include "bn254_io.h"
#include "bn254_pairing.h"
#include "bn254_pop.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_lane.h"
#include "bn254_host.h"

#define POP_WG 256
#define KERNEL_POP __global__ __launch_bounds__(POP_WG)
static inline unsigned pop_grid(size_t elems) { return (unsigned)((elems + POP_WG - 1) / POP_WG); }

// one element of the composer per lane: lane i of a wave stores message word base + i (bn254_pop.h)
KERNEL_POP void k_pop_compose(const uint32_t* pks, size_t n, PopMsgs out) {
  pop_compose_elem((size_t)blockIdx.x * POP_WG + threadIdx.x, n, pks, out);
}
KERNEL_POP void k_pop_fold(size_t n, uint8_t* first, const uint8_t* second) {
  pop_fold_elem((size_t)blockIdx.x * POP_WG + threadIdx.x, n, first, second);
}

// the context's buffer carved for n keys: [offsets n + 1 | messages 36 n words | key indices n | statuses n]; grown like the staging buffers
// (quiesce, free, allocate) before the call's first kernel
struct PopScratch { PopMsgs m; uint8_t* st; };
static int pop_scratch_reserve(bn254_ctx* c, size_t n, PopScratch* S) {
  const size_t off_bytes = (n + 1) * sizeof(uint64_t), msg_bytes = n * (size_t)BN_POP_MSG_BYTES, idx_bytes = n * sizeof(uint32_t);
  if (const int rc = scratch_reserve(c, &c->pop_buf, &c->pop_cap, off_bytes + msg_bytes + idx_bytes + n)) return rc;
  S->m.off = (uint64_t*)c->pop_buf;
  S->m.msgs = (uint32_t*)(c->pop_buf + off_bytes);
  S->m.key_idx = (uint32_t*)(c->pop_buf + off_bytes + msg_bytes);
  S->st = c->pop_buf + off_bytes + msg_bytes + idx_bytes;
  return 0;
}
static int launch_pop_compose(hipStream_t s, const uint8_t* d_pks, size_t n, const PopMsgs& out) {
  k_pop_compose<<<pop_grid(pop_compose_elems(n)), POP_WG, 0, s>>>((const uint32_t*)d_pks, n, out);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int launch_pop_fold(hipStream_t s, size_t n, uint8_t* first, const uint8_t* second) {
  k_pop_fold<<<pop_grid(n), POP_WG, 0, s>>>(n, first, second);
  HIP_TRY(hipGetLastError());
  return 0;
}

// These calls take no message buffer: a pending bn254_ctx_expect_msgs_len is neither consumed nor applied.  While the scope is open the entry
// points underneath see a call in progress (their MsgsLenScope leaves the declaration armed) and the hash kernels bound the composed buffer
// by its true length.
struct PopMsgsScope {
  bn254_ctx* c;
  uint64_t saved;
  PopMsgsScope(bn254_ctx* ctx, size_t n) : c(ctx), saved(ctx->msgs_len_call) {
    ++c->entry_depth;
    c->msgs_len_call = (uint64_t)n * BN_POP_MSG_BYTES;
  }
  ~PopMsgsScope() {
    c->msgs_len_call = saved;
    --c->entry_depth;
  }
  PopMsgsScope(const PopMsgsScope&) = delete;
  PopMsgsScope& operator=(const PopMsgsScope&) = delete;
};

// fail closed: until the proofs have been checked and the statuses folded, every way out of a registration leaves the context without keys
struct PopKeysGuard {
  bn254_ctx* c;
  bool keep = false;
  explicit PopKeysGuard(bn254_ctx* ctx) : c(ctx) {}
  ~PopKeysGuard() { if (!keep) c->n_keys = 0; }
  PopKeysGuard(const PopKeysGuard&) = delete;
  PopKeysGuard& operator=(const PopKeysGuard&) = delete;
};

extern "C" {

int bn254_batch_pop_verify_device(bn254_ctx* c, const uint8_t* d_pks, const uint8_t* d_pops, size_t n, uint32_t flags, uint8_t* d_status, void* stream) {
  if (!c || g1c_flag(flags) || (n && (!d_pks || !d_pops || !d_status)) || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_pks) || misaligned(d_pops)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  PopScratch S;
  if (const int rc = pop_scratch_reserve(c, n, &S)) return rc;
  PopMsgsScope msgs_scope(c, n);
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  {
    CallDone call_done(c, s);
    S.m.key_idx = nullptr;
    if (const int rc = launch_pop_compose(s, d_pks, n, S.m)) return rc;
  }
  // the verify itself, slicing (ws_chunk_for) included: the offsets are absolute, a slice is the same arrays further in
  return bn254_batch_verify_device(c, (const uint8_t*)S.m.msgs, S.m.off, d_pops, d_pks, n, flags | BN254_FLAG_G2_SUBGROUP_CHECK, d_status, stream);
}
int bn254_batch_pop_verify(bn254_ctx* c, const uint8_t* pks, const uint8_t* pops, size_t n, uint32_t flags, uint8_t* status) {
  if (!c || g1c_flag(flags) || (n && (!pks || !pops || !status)) || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t *d_pops = st.in(2, pops, n * 64), *d_pks = st.in(3, pks, n * 128);
  uint8_t* d_status = st.out(4, n, status);
  if (st.ok()) st.rc = bn254_batch_pop_verify_device(c, d_pks, d_pops, n, flags, d_status, nullptr);
  return st.finish();
}

int bn254_batch_pop_prove_device(bn254_ctx* c, const uint8_t* d_sks, size_t n, uint8_t* d_pks, uint8_t* d_pops, uint8_t* d_status, void* stream) {
  if (!c || (n && (!d_sks || !d_pks || !d_pops || !d_status)) || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_sks) || misaligned(d_pks) || misaligned(d_pops)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  PopScratch S;
  int rc = pop_scratch_reserve(c, n, &S);
  if (rc) return rc;
  PopMsgsScope msgs_scope(c, n);
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  if ((rc = bn254_batch_g2_mul_device(c, nullptr, d_sks, n, 1, d_pks, d_status, stream))) return rc;        // PublicKey::from_private_key
  S.m.key_idx = nullptr;
  if ((rc = launch_pop_compose(s, d_pks, n, S.m))) return rc;
  // sign reserves one workspace entry per item and does not slice: the slices are cut here, by the verify's rule
  size_t chunk = ws_chunk_for(c, n);
  if (chunk == 0) chunk = n;
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t len = n - lo < chunk ? n - lo : chunk;
    if ((rc = bn254_batch_sign_device(c, (const uint8_t*)S.m.msgs, S.m.off + lo, d_sks + 32 * lo, len, d_pops + 64 * lo, S.st + lo, stream))) return rc;
  }
  return launch_pop_fold(s, n, d_status, S.st);
}
int bn254_batch_pop_prove(bn254_ctx* c, const uint8_t* sks, size_t n, uint8_t* pks, uint8_t* pops, uint8_t* status) {
  if (!c || (n && (!sks || !pks || !pops || !status)) || n > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HostStaging st(c);
  const uint8_t* d_sks = st.in(0, sks, n * 32);
  uint8_t *d_pks = st.out(1, n * 128, pks), *d_pops = st.out(2, n * 64, pops), *d_status = st.out(3, n, status);
  if (st.ok()) st.rc = bn254_batch_pop_prove_device(c, d_sks, n, d_pks, d_pops, d_status, nullptr);
  return st.finish();
}

int bn254_ctx_register_keys_pop(bn254_ctx* c, const uint8_t* pks, const uint8_t* pops, size_t n_keys, uint32_t flags, uint8_t* key_status) {
  if (!c || g1c_flag(flags) || (n_keys && (!pks || !pops)) || n_keys > 0xFFFFFFFFu) return BN254_E_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  int rc = register_keys_begin(c, n_keys);
  if (rc) return rc;
  if (n_keys == 0) return 0;
  PopKeysGuard guard(c);
  PopScratch S;
  if ((rc = pop_scratch_reserve(c, n_keys, &S))) return rc;
  size_t chunk = ws_chunk_for(c, n_keys);
  if (chunk == 0) chunk = n_keys;
  if ((rc = ws_reserve(c, chunk))) return rc;
  PopMsgsScope msgs_scope(c, n_keys);
  HostStaging st(c);
  const uint8_t *d_pops = st.in(2, pops, n_keys * 64), *d_pks = st.in(3, pks, n_keys * 128);
  st.copy_back(key_status, c->key_st, n_keys);
  if (!st.ok()) return st.rc;
  hipStream_t s = c->stream;
  if ((rc = launch_register_keys(c, d_pks, n_keys, flags))) return rc;
  if ((rc = launch_pop_compose(s, d_pks, n_keys, S.m))) return rc;
  c->n_keys = n_keys;                                  // what the keyed route reads its table through; the guard takes it back on every early return
  for (size_t lo = 0; lo < n_keys; lo += chunk) {
    const size_t len = n_keys - lo < chunk ? n_keys - lo : chunk;
    if ((rc = launch_decode_g1(c, s, d_pops + 64 * lo, len, flags & BN254_FLAG_REJECT_IDENTITY, PL_P1X, BY_P1_INF, 0))) return rc;
    if ((rc = launch_hash_rounds(c, s, (const uint8_t*)S.m.msgs, S.m.off + lo, len, PL_P2X, BY_P2_INF, nullptr))) return rc;
    if ((rc = launch_keyed_miller_fe(c, s, len, S.m.key_idx + lo, S.st + lo, ctx_key_table(c), c->key_xy))) return rc;
  }
  if ((rc = launch_pop_fold(s, n_keys, c->key_st, S.st))) return rc;
  if ((rc = st.finish())) return rc;
  guard.keep = true;
  return 0;
}

}  // extern "C"
