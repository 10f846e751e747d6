// The key-table BUILDER of the exact verify's key dedup (bn254_keydedup.hip: k_kd_lines) as a program of the lane machine's wave T
// (bn254_lmachine.h): one key on nine lane pairs, its register file in LDS, doubling in two product levels and a mixed addition in three.
//
// kd_walk_raw_lines (bn254_keydedup.h) runs g2_line_table's walk on ONE lane pair: ~12 products in sequence per doubling step, 87 steps.
// Here every product of a dependency level runs in its own lane pair, the depth of the walk falls to 1 + 2 * 64 + 3 * 25 = 204 levels.
// Wave T's formulas are dbl_step / add_step expanded (w = 3b' z beside the point), the same polynomials of (x, y, z): the point after every
// step is the SAME field element as g2_line_table's, and so are the raw lines this program hands out:
//   doubling  (c0, c1, c2) = (h = 2 y z, -3 x^2, b - e)        = slots HOA, HOB, HOC after level 0
//   addition  (c0, c1, c2) = (mu, -theta, theta x_Q - mu y_Q)  = slots HOB, KD_C1, KD_C2 after level 0, with theta x_Q - mu y_Q = y x_Q - x y_Q
//             (the z terms cancel), two products that level 0 of wave T leaves room for.
// kd_scale_line then gives, word for word, the table of registration (c0 / c2, c1 / c2, canonical limbs), and a line has c2 = 0 here
// exactly when it has in g2_line_table.  Every linear output is weakly reduced (fp_lin4_reduce): every slot is tight, within +-0.52 q; the
// bound proof is the interval tracker's run of the host model below (tests/test_kd_builder.py).
// The builder runs one wave alone: a level's stages are ordered by wavefront fences, slots are never relocated (parity 0 throughout).
// Include after bn254_pairing.h and bn254_lmachine.h (pair layout: BN_SPLIT_FP2).
#pragma once

namespace bn254 {

// builder-only slots: wave L's temporaries (no wave L runs beside the builder)
enum {
  LS_KD_YQX = LS_LL0,            // y x_Q
  LS_KD_XQY = LS_LL1,            // x y_Q
  LS_KD_C1 = LS_LM0,             // -theta
  LS_KD_C2 = LS_LM1,             // y x_Q - x y_Q
  LS_KD_SLOTS = LS_REL0 + LS_REL_N // slots the builder's register file needs (the hand-over block of parity 0 is the last it touches)
};
// level 0 of an addition: wave T's (theta, mu) plus the line's c1 and c2
LM_TABLE LM_KD_ADD0[1][9] = {{
    LM_E(lm_mul(LS_T1, LS_TQY, LS_TZ), lm_lin(LS_HOA, LS_TY, 1, LS_T1, -1)),
    LM_E(lm_mul(LS_T2, LS_TQX, LS_TZ), lm_lin(LS_HOB, LS_TX, 1, LS_T2, -1)),
    LM_E(lm_mul(LS_KD_YQX, LS_TY, LS_TQX), lm_lin(LS_KD_C2, LS_KD_YQX, 1, LS_KD_XQY, -1)),
    LM_E(lm_mul(LS_KD_XQY, LS_TX, LS_TQY), lm_lin(LS_KD_C1, LS_T1, 1, LS_TY, -1)),
    LM_E(LM_NOP_P, LM_NOP_L), LM_E(LM_NOP_P, LM_NOP_L), LM_E(LM_NOP_P, LM_NOP_L), LM_E(LM_NOP_P, LM_NOP_L), LM_E(LM_NOP_P, LM_NOP_L)}};

// the levels of the program, and the slots of a step's raw line (c0, c1, c2)
enum KdLevel { KD_LV_INIT = 0, KD_LV_D0, KD_LV_D1, KD_LV_A0, KD_LV_A1, KD_LV_A2, KD_LV_N };
enum { KD_LO_DBL = 0, KD_LO_ADD = 1 };
BN_DEV int kd_line_slot(int kind, int coef) {
  return kind == KD_LO_DBL ? (coef == 0 ? LS_HOA : coef == 1 ? LS_HOB : LS_HOC) : (coef == 0 ? LS_HOB : coef == 1 ? LS_KD_C1 : LS_KD_C2);
}
// slots the caller fills before the program: ONE, B3, PKX, PKY, CPKX, CPKY, FX1, FY1, FX2 (LM_T_INIT derives pi(Q), pi^2(Q).x, -Q.y, T)
template <class Box> BN_DEV void kd_builder_init(Box& bx, const G2Affine& q) {
  bx.put(bx.slot(LS_ONE), fp2_one()); bx.put(bx.slot(LS_B3), fp2_load_const(C_TWIST_3B));
  bx.put(bx.slot(LS_PKX), q.x); bx.put(bx.slot(LS_PKY), q.y); bx.put(bx.slot(LS_CPKX), fp2_conj(q.x)); bx.put(bx.slot(LS_CPKY), fp2_conj(q.y));
  bx.put(bx.slot(LS_FX1), fp2_load_const(C_TW_FROB_X1)); bx.put(bx.slot(LS_FY1), fp2_load_const(C_TW_FROB_Y1));
  bx.put(bx.slot(LS_FX2), fp2_load_const(C_TW_FROB_X2));
}
// the walk of g2_line_table as levels: M provides level(KdLevel), add_point(qx slot, qy slot) (TQX, TQY <- the point; ordered before the
// next level) and line(idx, kind) (the raw line of step idx is in the slots kd_line_slot(kind, 0 .. 2))
template <class M> BN_DEV void kd_builder_program(M& m) {
  m.level(KD_LV_INIT);
  int idx = 0;
#if defined(__HIPCC__)
#pragma clang loop unroll(disable)
#endif
  for (int d = 0; d < 64; ++d) {
    m.level(KD_LV_D0); m.level(KD_LV_D1); m.line(idx++, KD_LO_DBL);
    const int digit = C_ATE_NAF[d];                         // uniform: a public constant
    if (digit != 0) {
      m.add_point(LS_PKX, digit > 0 ? LS_PKY : LS_NPKY);
      m.level(KD_LV_A0); m.level(KD_LV_A1); m.level(KD_LV_A2); m.line(idx++, KD_LO_ADD);
    }
  }
  m.add_point(LS_Q1X, LS_Q1Y); m.level(KD_LV_A0); m.level(KD_LV_A1); m.level(KD_LV_A2); m.line(idx++, KD_LO_ADD);
  m.add_point(LS_Q2X, LS_PKY); m.level(KD_LV_A0); m.level(KD_LV_A1); m.level(KD_LV_A2); m.line(idx++, KD_LO_ADD);
}
#if defined(__HIPCC__)
__device__ __forceinline__ const LmEntry* kd_level_table(int lv) {
  return lv == KD_LV_INIT ? LM_T_INIT[0] : lv == KD_LV_D0 ? LM_T_DBL[0] : lv == KD_LV_D1 ? LM_T_DBL[1] : lv == KD_LV_A0 ? LM_KD_ADD0[0]
       : lv == KD_LV_A1 ? LM_T_ADD[1] : LM_T_ADD[2];
}
#else
inline const LmEntry (&kd_level_table(int lv))[9] {
  return lv == KD_LV_INIT ? LM_T_INIT[0] : lv == KD_LV_D0 ? LM_T_DBL[0] : lv == KD_LV_D1 ? LM_T_DBL[1] : lv == KD_LV_A0 ? LM_KD_ADD0[0]
       : lv == KD_LV_A1 ? LM_T_ADD[1] : LM_T_ADD[2];
}
// ---- host model: the builder's program on LmHostBox (nine pairs of a stage one after the other); emit(idx, c0, c1, c2) per line.
// Returns true if some line has c2 = 0 (as kd_walk_raw_lines).
template <class Emit> bool kd_builder_model(const G2Affine& q, Emit&& emit) {
  static LmHostBox bx;
  for (int i = 0; i < LS_COUNT; ++i) bx.s[i] = fp2_zero();
  kd_builder_init(bx, q);
  struct M {
    LmHostBox& bx;
    Emit& emit;
    bool degenerate;
    void level(int lv) { lm_host_level(bx, kd_level_table(lv), 0, false, false); }
    void add_point(int qx, int qy) { bx.s[LS_TQX] = bx.s[qx]; bx.s[LS_TQY] = bx.s[qy]; }
    void line(int idx, int kind) {
      const Fp2 c2 = bx.s[kd_line_slot(kind, 2)];
      degenerate = fp2_is_zero(c2) || degenerate;
      emit(idx, bx.s[kd_line_slot(kind, 0)], bx.s[kd_line_slot(kind, 1)], c2);
    }
  } m{bx, emit, false};
  kd_builder_program(m);
  return m.degenerate;
}
#endif

}  // namespace bn254
