// The arithmetic of the per-call key tables (bn254_keydedup.hip) in the PAIR layout, shared by the device kernels and their host emulation
// (tests/test_keydedup_tables.py: word-for-word parity with g2_line_table + fp_canon, bound proof under -DBN_TRACK_BOUNDS).
// g2_line_table (bn254_pairing.h) computes a key's 87 lines and scales each one by its own c2^-1 on the spot: 87 inversions in sequence.
// Here the walk and the scaling are split — kd_walk_raw_lines emits the raw (c0, c1, c2) of every line, kd_scale_line turns one of them
// into the c2 = 1 form with canonical limbs.  The device scales the 87 lines of a key with ONE inversion (k_kd_scale: Montgomery's trick as a
// product tree over the key's c2 values); kd_scale_tree below is that tree's host form, equal to kd_scale_line line by line.  Same operations at the same
// norm sites (290 .. 293) as g2_line_table: the same values and the same bounds.  kd_walk_raw_lines is the reference formulation of the
// walk (one lane pair, one step after the other); the device builder runs the same walk as the lane machine's level program
// (bn254_kdlines.h), whose raw lines tests/test_kd_builder.py checks against it.
// Include after bn254_pairing.h (pair layout: BN_SPLIT_FP2).
#pragma once

namespace bn254 {

// the twist-point walk of g2_line_table; emit(idx, c0, c1, c2) per line; returns true if some line has c2 = 0 (no table for this key)
template <class Emit>
BN_DEV bool kd_walk_raw_lines(const G2Affine& q, Emit&& emit) {
  G2Proj t;
  LineCoef l;
  t.x = q.x; t.y = q.y; t.z = fp2_one();
  const Fp2 q_yneg = fp2_neg(q.y);
  bool degenerate = false;
  int idx = 0;
  auto line = [&]() {
    const Fp2 c2 = NR(290, l.c2);
    degenerate = fp2_is_zero(c2) || degenerate;
    emit(idx++, NS(292, l.c0), NS(293, l.c1), c2);
  };
#if defined(__HIPCC__)
#pragma clang loop unroll(disable)
#endif
  for (int d = 0; d < 64; ++d) {
    dbl_step(t, l); line();
    const int digit = C_ATE_NAF[d];
    if (digit != 0) { add_step(t, l, q.x, fp2_select(digit > 0, q.y, q_yneg)); line(); }
  }
  add_step(t, l, fp2_mul(fp2_conj(q.x), fp2_load_const(C_TW_FROB_X1)), fp2_mul(fp2_conj(q.y), fp2_load_const(C_TW_FROB_Y1))); line();
  add_step(t, l, fp2_mul(q.x, fp2_load_const(C_TW_FROB_X2)), q.y); line();
  return degenerate;
}
// one raw line into the table form: (c0 / c2, c1 / c2), canonical limbs (what k_register_keys stores)
BN_DEV void kd_scale_line(const Fp2& c0, const Fp2& c1, const Fp2& c2, Fp2& r0, Fp2& r1) {
  const Fp2 inv = NS(291, fp2_inv(c2));
  const Fp2 a = fp2_mul(c0, inv), b = fp2_mul(c1, inv);
  BN_FOR_ROLES(k) { r0.c[k] = fp_canon(a.c[k]); r1.c[k] = fp_canon(b.c[k]); }
}

// The tree of k_kd_scale (bn254_keydedup.hip), operation for operation: heap order, node 1 = the root, leaves KD_TREE_LEAVES + line (ones
// beyond the 87 lines); leaf = the weakly reduced raw c2 (site 290's default); KD_TREE_LEVELS product levels up; fp2_inv of the root; the same
// number of levels down (inverse of a node = inverse of its parent x its sibling); then kd_scale_line's two products and fp_canon.  Exact
// field arithmetic and canonical results: the words are kd_scale_line's.  A zero c2 makes the root zero; the results of such a key are not
// used (KD_DEGENERATE) and the work stays finite.
#define KD_TREE_LEAVES 128
#define KD_TREE_LEVELS 7
#if !defined(__HIPCC__)
static inline void kd_scale_tree(const Fp2* c0, const Fp2* c1, const Fp2* c2, Fp2* r0, Fp2* r1) {   // BN_N_FIXED_LINES entries each
  static_assert(BN_N_FIXED_LINES <= KD_TREE_LEAVES && (1 << KD_TREE_LEVELS) == KD_TREE_LEAVES, "tree shape");
  Fp2 prod[2 * KD_TREE_LEAVES], inv[2 * KD_TREE_LEAVES];
  for (int p = 0; p < KD_TREE_LEAVES; ++p) prod[KD_TREE_LEAVES + p] = p < BN_N_FIXED_LINES ? fp2_reduce_weak(c2[p]) : fp2_one();
  for (int w = KD_TREE_LEAVES / 2; w >= 1; w >>= 1)
    for (int node = w; node < 2 * w; ++node) prod[node] = fp2_mul(prod[2 * node], prod[2 * node + 1]);
  inv[1] = fp2_inv(prod[1]);
  for (int w = 2; w <= KD_TREE_LEAVES; w <<= 1)
    for (int node = w; node < 2 * w; ++node) inv[node] = fp2_mul(inv[node >> 1], prod[node ^ 1]);
  for (int p = 0; p < BN_N_FIXED_LINES; ++p) {
    const Fp2 a = fp2_mul(c0[p], inv[KD_TREE_LEAVES + p]), b = fp2_mul(c1[p], inv[KD_TREE_LEAVES + p]);
    BN_FOR_ROLES(k) { r0[p].c[k] = fp_canon(a.c[k]); r1[p].c[k] = fp_canon(b.c[k]); }
  }
}
#endif

// FOLDED ROWS.  At a nonzero digit of the loop (and at its end) two lines of the same key multiply f with no squaring between them, both
// evaluated at the same G1 point (x, y) and both in the c2 = 1 form, so their product is a five-term element whose Fq2 coefficients
// depend on the key alone (w^6 = xi):
//   (c0 y + c1 x w + w^3)(c0' y + c1' x w + w^3) = (K0 y^2 + xi) + K1 xy w + K2 x^2 w^2 + K3 y w^3 + K4 x w^4
//   K0 = c0 c0', K1 = c0 c1' + c1 c0' (Karatsuba: (c0 + c1)(c0' + c1') - K0 - K2), K2 = c1 c1', K3 = c0 + c0', K4 = c1 + c1'
// kd_fold_pair is that one row from two canonical table lines, canonical again (sites 294 / 295: the two Karatsuba sums of canonical
// limbs); the tail of k_kd_scale runs it on the lane pairs of a key's BN_N_FOLD_ROWS rows (bn254_constants.h: C_FOLD_FIRST), and
// miller_loop_keyed_fold (bn254_pairing.h) reads the rows.
BN_DEV void kd_fold_pair(const Fp2& c0, const Fp2& c1, const Fp2& d0, const Fp2& d1, Fp2 k[5]) {
  const Fp2 k0 = fp2_mul(c0, d0), k2 = fp2_mul(c1, d1);
  const Fp2 k1 = fp2_sub(fp2_sub(fp2_mul(NS(294, fp2_add(c0, c1)), NS(295, fp2_add(d0, d1))), k0), k2);
  const Fp2 k3 = fp2_add(c0, d0), k4 = fp2_add(c1, d1);
  BN_FOR_ROLES(r) { k[0].c[r] = fp_canon(k0.c[r]); k[1].c[r] = fp_canon(k1.c[r]); k[2].c[r] = fp_canon(k2.c[r]); k[3].c[r] = fp_canon(k3.c[r]); k[4].c[r] = fp_canon(k4.c[r]); }
}
#if !defined(__HIPCC__)
// a key's BN_N_FOLD_ROWS folded rows from its BN_N_FIXED_LINES canonical (c0, c1) rows: the host form of k_kd_scale's tail
static inline void kd_fold_lines(const Fp2* c0, const Fp2* c1, Fp2 (*fold)[5]) {
  for (int r = 0; r < BN_N_FOLD_ROWS; ++r) {
    const int i = C_FOLD_FIRST[r];
    kd_fold_pair(c0[i], c1[i], c0[i + 1], c1[i + 1], fold[r]);
  }
}
#endif

#if defined(__HIPCC__)
// One uncompressed G2 point (/root/reference/src/utils.rs:107-116) on a lane pair: each lane reads, range-checks and converts the two
// 32-byte words of its role; identity, range and curve rules combined over the pair.  The status of k_decode_g2_pair before its optional
// subgroup ladder — the one decode both that kernel and the key-table builder run, so their statuses cannot drift apart.
BN_DEV bool load_fp_be_checked(Fp& r, const uint8_t* p, uint32_t& any) {
  const uint32_t* w = (const uint32_t*)p;
  U256 t;
#pragma unroll
  for (int k = 0; k < 8; ++k) { t.w[7 - k] = __builtin_bswap32(w[k]); any |= w[k]; }
  bool ok = !u256_geq(t.w, C_Q);
  r = fp_from_u256(t);
  return ok;
}
BN_DEV uint8_t decode_g2_pair_role(G2Affine& q, const uint8_t* b, uint32_t flags) {
  const unsigned role = threadIdx.x & 1u;
  uint32_t any = 0;
  bool ok = load_fp_be_checked(q.x.c[0], b + 32 * role, any);
  ok = load_fp_be_checked(q.y.c[0], b + 64 + 32 * role, any) && ok;
  any |= (uint32_t)bn_partner_word((int32_t)any);
  ok = bn_pair_and(ok);
  q.inf = any == 0;
  uint8_t st = ST_OK;
  if (q.inf) st = (flags & FLAG_REJECT_IDENTITY) ? (uint8_t)ST_INVALID_GROUP_POINT : (uint8_t)ST_OK;
  else if (!ok) st = ST_NOT_MEMBER;
  const bool on_curve = g2_on_curve(q);             // pair-combined; evaluated by every lane
  if (st == ST_OK && !q.inf && !on_curve) st = ST_INVALID_GROUP_POINT;
  return st;
}
#endif

}  // namespace bn254
