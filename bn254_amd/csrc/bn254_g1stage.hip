// Translation unit of libbn254hip.so: compressed G1 input of the registered-key calls (include/bn254_hip.h: BN254_FLAG_G1_COMPRESSED;
// DESIGN.md §10p) and bn254_batch_g1_decompress_device.  A call under the flag stages its 33-byte encodings ONCE, at its outermost entry:
// one lane per item decompresses (G1::from_compressed as Signature::from_compressed uses it, the reference's src/types.rs:233-237 and
// src/utils.rs:84-104) into the 64 bytes the call's existing route then reads — the point, or a stand-in no decoder accepts — and keeps the
// item's own status beside it; behind the call one lane per item puts that status where the route reported the stand-in (bn254_host.h:
// g1c_call).  The per-item bodies are bn254_g1stage.h, shared with the CPU suite's host compilation.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/bn254_hip.h"
#include "bn254_io.h"
#include "bn254_g1stage.h"

using namespace bn254;

#include "bn254_ws.h"
#include "bn254_host.h"

// lane per item; the square root is the same straight-line chain in every lane, so a wave with failing items does not diverge in it
KERNEL_SMALL void k_g1c_stage(const uint8_t* in33, size_t n, uint8_t* out64, uint8_t* pre) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  pre[i] = g1c_stage_item(out64 + 64 * i, in33 + 33 * i);
}
KERNEL_SMALL void k_g1c_overlay(size_t n, const uint8_t* pre, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  const uint8_t p = pre[i];
  if (p != ST_OK) status[i] = g1c_overlay_item(status[i], p);
}
KERNEL_SMALL void k_g1c_decompress(const uint8_t* in33, size_t n, uint8_t* out64, uint8_t* status) {
  const size_t i = (size_t)blockIdx.x * BN_WAVE + threadIdx.x;
  if (i >= n) return;
  status[i] = g1c_decompress_item(out64 + 64 * i, in33 + 33 * i);
}

int g1c_reserve(bn254_ctx* c, size_t n) { return scratch_reserve(c, &c->g1c_buf, &c->g1c_cap, 65 * n); }
int g1c_stage(bn254_ctx* c, hipStream_t s, const uint8_t* d_in33, size_t n) {
  if (65 * n > c->g1c_cap) return BN254_E_BAD_ARGUMENT;                  // the caller reserves before its first kernel
  k_g1c_stage<<<grid_for(n), BN_WAVE, 0, s>>>(d_in33, n, c->g1c_buf, g1c_pre(c, n));
  HIP_TRY(hipGetLastError());
  return 0;
}
int g1c_overlay(bn254_ctx* c, hipStream_t s, size_t n, uint8_t* d_status) {
  k_g1c_overlay<<<grid_for(n), BN_WAVE, 0, s>>>(n, g1c_pre(c, n), d_status);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

int bn254_batch_g1_decompress_device(bn254_ctx* c, const uint8_t* d_in33, size_t n, uint8_t* d_out64, uint8_t* d_status, void* stream) {
  if (!c || n > 0xFFFFFFFFu || (n && (!d_in33 || !d_out64 || !d_status))) return BN254_E_BAD_ARGUMENT;
  if (n == 0) return 0;
  if (misaligned(d_out64)) return BN254_E_MISALIGNED;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  CallDone call_done(c, s);
  k_g1c_decompress<<<grid_for(n), BN_WAVE, 0, s>>>(d_in33, n, d_out64, d_status);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
