// The G1 side of the randomised batch verification of keyed aggregates over distinct messages (bn254_aggrand.hip), as device functions a
// host-simulation harness compiles too (tests/test_aggregate_distinct_keyed_randomized.py builds it).  Include after bn254_curve.h and
// bn254_hash.h.
//
// Aggregate i (lo_i = agg_off[i]) belongs to GROUP lo_i / G, bucket (g, key) = g (K + 1) + key with K = the registered keys; key K is the
// signature's bucket, whose table is -G2's (the entry K behind the keys).  A group with ONE aggregate at the check takes r = 1.
#pragma once

#define AGGR_NONE 0xFFFFFFFFu

BN_DEV uint64_t aggr_group(uint64_t lo, uint64_t G) { return lo / G; }
BN_DEV uint64_t aggr_bucket(uint64_t g, uint32_t key, uint32_t n_keys) { return g * ((uint64_t)n_keys + 1) + key; }

// r_i * p as a Jacobian point: r_i from rand_scalar (bn254_hash.h) with i = the aggregate's index, mode 0 = 128-bit, 1 = 64-bit, 2 = GLV
// (k1 + k2 lambda); one = 1: the point itself (a group with one aggregate at the check).  `acc` may live in LDS (the ladders work in place).
BN_DEV void aggr_scale(G1Jac& acc, const G1Affine& p, const uint32_t* seed_be, uint64_t i, int mode, bool one) {
  if (one) { jac_from_affine(acc, p); return; }
  uint32_t k[4];
  rand_scalar(k, seed_be, i, mode == 1);
  if (mode == 2) g1_mul_glv(acc, p, k, k + 2); else if (mode == 1) jac_mul_u64(acc, p, k); else jac_mul_u128(acc, p, k);
  if (p.inf) jac_set_identity(acc);                    // the ladders read the coordinates only (an identity signature)
}
