// hostsim_pooltab — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the builders of the aggregate verify's subset-sum tables (bn254_amd/csrc/bn254_pooltab.h: the very functions
// k_pool_subsets_g2 / _g1, k_pool_pairs_g1, k_pool_quads_g1, k_pool_widen_g1 / _g2 run), in the one-lane layout they run in, lane after
// lane, in the launch order of agg_build_tables.  Built plain and with -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated limb /
// value bound, and on a table entry outside the stored-word contract) by tests/test_aggregate_pool_tables.py.  -DPT_PAIR_CONSUMER: the pair
// layout instead, both lane roles in sequence — the consumer's side only: jac_from_affine and jac_accumulate_from on records loaded under
// the contract, as k_aggregate_pair runs them.
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(PT_PAIR_CONSUMER)
#define BN_SPLIT_FP2 1
#endif
#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_pairing.h"
#include "../../bn254_amd/csrc/bn254_pooltab.h"

using namespace bn254;

static Fp fp_from_be32(const uint8_t* b) {
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = ((uint32_t)b[28 - 4 * i] << 24) | ((uint32_t)b[29 - 4 * i] << 16) | ((uint32_t)b[30 - 4 * i] << 8) | b[31 - 4 * i];
  return fp_from_u256(x);
}
static void fp_to_be32(uint8_t* b, const Fp& a) {
  U256 x = fp_to_u256(a);
  for (int i = 0; i < 8; ++i) { b[28 - 4 * i] = (uint8_t)(x.w[i] >> 24); b[29 - 4 * i] = (uint8_t)(x.w[i] >> 16); b[30 - 4 * i] = (uint8_t)(x.w[i] >> 8); b[31 - 4 * i] = (uint8_t)x.w[i]; }
}
static bool all_zero(const uint8_t* b, int n) { uint8_t o = 0; for (int i = 0; i < n; ++i) o |= b[i]; return o == 0; }

// a table: `entries` records and one more behind them that nothing may write (the canary), every word preset to a pattern no builder leaves
struct HostTab {
  std::vector<int32_t> planes;
  std::vector<uint8_t> st;
  size_t entries = 0;
  uint32_t g2 = 0;
  void reset(size_t n, uint32_t is_g2) {
    entries = n; g2 = is_g2;
    planes.assign((n + 1) * (is_g2 ? 2 : 1) * PT_HALF_WORDS, 0x5A5A5A5A);
    st.assign(n + 1, 0x5A);
  }
  PtTab tab() { return PtTab{planes.data(), st.data(), g2}; }
  bool canary_ok() const {
    if (entries == 0 && planes.empty()) return true;
    const size_t w = (g2 ? 2 : 1) * PT_HALF_WORDS;
    for (size_t k = 0; k < w; ++k) if (planes[entries * w + k] != 0x5A5A5A5A) return false;
    return st[entries] == 0x5A;
  }
};
// raw words of a coordinate the tests hand over as canonical bytes (a decoded pool entry: in [0, q), inside the contract by construction)
static void put_canonical(const PtTab& t, int e, size_t j, const uint8_t* be32) {
  const Fp a = fp_from_be32(be32);
  int32_t* w = t.planes + pt_word(t, e, j);
  for (int k = 0; k < BN_LIMBS; ++k) w[k] = a.v[k];
}
static void put_const(const PtTab& t, int e, size_t j, const int32_t* c) {
  int32_t* w = t.planes + pt_word(t, e, j);
  for (int k = 0; k < BN_LIMBS; ++k) w[k] = c[k];
}

#if !defined(PT_PAIR_CONSUMER)
static HostTab g_tab[8];            // indexed as the context's pools: 0 keys, 1 signatures, 3 T8 keys, 4 T4, 5 T16, 6 T8 signatures, 7 T2
static size_t g_n_msgs, g_n_signers, g_n_groups, g_groups4, g_groups2, g_n_chunks;

// a pool entry as k_pool_decode_g1 / _g2 leave it: st = the decode status the test hands over | 0x80 for the identity (all-zero bytes); the
// generator's coordinates under a non-zero decode status
static void decode_pool_g1(const PtTab& t, size_t j, const uint8_t* b, uint8_t status) {
  const bool inf = status == 0 && all_zero(b, 64);
  if (status != 0) { put_const(t, 0, j, C_G1_GEN[0]); put_const(t, 1, j, C_G1_GEN[1]); }
  else { put_canonical(t, 0, j, b); put_canonical(t, 1, j, b + 32); }
  t.st[j] = (uint8_t)(status | (inf ? 0x80 : 0));
}
static void decode_pool_g2(const PtTab& t, size_t j, const uint8_t* b, uint8_t status) {
  const bool inf = status == 0 && all_zero(b, 128);
  if (status != 0) { put_const(t, 0, j, C_G2_GEN[0][0]); put_const(t, 1, j, C_G2_GEN[0][1]); put_const(t, 2, j, C_G2_GEN[1][0]); put_const(t, 3, j, C_G2_GEN[1][1]); }
  else for (int e = 0; e < 4; ++e) put_canonical(t, e, j, b + 32 * e);
  t.st[j] = (uint8_t)(status | (inf ? 0x80 : 0));
}
// every lane of a launch of `total` live lanes, then one lane past the end (it must store nothing)
template <class Fn> static void launch(size_t total, Fn fn) { for (size_t lane = 0; lane <= total; ++lane) fn(lane); }

extern "C" {

// The pools (n_signers keys of 128 bytes, n_msgs x n_signers signatures of 64; *_st: the decode status of each entry, 0 = it decodes) and
// every table built from them, in the order of agg_build_tables.  t4_route: 0 = T4 from pairs + quads, 1 = from pt_subsets_g1_lane (T2 is
// then not built).
void hp_build(size_t n_msgs, size_t n_signers, const uint8_t* pks, const uint8_t* pk_st, const uint8_t* sigs, const uint8_t* sig_st, int t4_route) {
  g_n_msgs = n_msgs; g_n_signers = n_signers;
  g_n_groups = (n_signers + 7) / 8; g_groups4 = 2 * g_n_groups; g_groups2 = 2 * g_groups4; g_n_chunks = (g_n_groups + 1) / 2;
  for (auto& t : g_tab) t = HostTab();
  g_tab[0].reset(n_signers, 1); g_tab[1].reset(n_msgs * n_signers, 0);
  const PtTab pk = g_tab[0].tab(), sg = g_tab[1].tab();
  for (size_t j = 0; j < n_signers; ++j) decode_pool_g2(pk, j, pks + 128 * j, pk_st[j]);
  for (size_t j = 0; j < n_msgs * n_signers; ++j) decode_pool_g1(sg, j, sigs + 64 * j, sig_st[j]);
  g_tab[3].reset(g_n_groups * 256, 1);
  const PtTab t8k = g_tab[3].tab();
  launch(g_n_groups * 256, [&](size_t lane) { pt_subsets_g2_lane(lane, pk, n_signers, g_n_groups, t8k); });
  g_tab[4].reset(n_msgs * g_groups4 * 16, 0);
  const PtTab t4 = g_tab[4].tab();
  if (t4_route == 0) {
    g_tab[7].reset(n_msgs * g_groups2 * 4, 0);
    const PtTab t2 = g_tab[7].tab();
    launch(n_msgs * g_groups2, [&](size_t lane) { pt_pairs_g1_lane(lane, sg, n_signers, g_groups2, n_msgs, t2); });
    launch(n_msgs * g_groups4 * 4, [&](size_t lane) { pt_quads_g1_lane(lane, t2, g_groups2, g_groups4, n_msgs, t4); });
  } else {
    launch(n_msgs * g_groups4 * 16, [&](size_t lane) { pt_subsets_g1_lane(lane, sg, n_signers, g_groups4, n_msgs, t4); });
  }
  g_tab[5].reset(g_n_chunks * 65536, 1);
  const PtTab t16 = g_tab[5].tab();
  launch(g_n_chunks * 256 * (256 / BN_WIDEN_G2_NLO), [&](size_t lane) { pt_widen_g2_lane(lane, t8k, g_n_groups, g_n_chunks, t16); });
  g_tab[6].reset(n_msgs * g_n_groups * 256, 0);
  const PtTab t8s = g_tab[6].tab();
  launch(n_msgs * g_n_groups * 16, [&](size_t lane) { pt_widen_g1_lane(lane, t4, g_groups4, g_n_groups, n_msgs, t8s); });
}
size_t hp_entries(int which) { return which >= 0 && which < 8 ? g_tab[which].entries : 0; }
int hp_canaries_ok(void) { for (auto& t : g_tab) if (!t.canary_ok()) return 0; return 1; }
// entries first .. first + count - 1 of table `which` as the device hook hands them out: canonical bytes (64 per G1 entry, 128 per G2 entry,
// zeros under the identity flag) and the raw status bytes.  Returns 0, or -1 for a range outside the table.
int hp_read(int which, size_t first, size_t count, uint8_t* points, uint8_t* flags) {
  if (which < 0 || which > 7 || first > g_tab[which].entries || count > g_tab[which].entries - first) return -1;
  const PtTab t = g_tab[which].tab();
  for (size_t i = 0; i < count; ++i) {
    const size_t j = first + i;
    flags[i] = t.st[j];
    if (t.g2) {
      G2Affine q;
      pool_load_aff(t, j, q);
      uint8_t* o = points + 128 * i;
      if (q.inf) { memset(o, 0, 128); continue; }
      fp_to_be32(o, q.x.c0); fp_to_be32(o + 32, q.x.c1); fp_to_be32(o + 64, q.y.c0); fp_to_be32(o + 96, q.y.c1);
    } else {
      G1Affine p;
      pool_load_aff(t, j, p);
      uint8_t* o = points + 64 * i;
      if (p.inf) { memset(o, 0, 64); continue; }
      fp_to_be32(o, p.x); fp_to_be32(o + 32, p.y);
    }
  }
  return 0;
}

// ONE lane of the widening on operands of the caller's choice: out[i] = A + B[i] for i < batch (4 or 8), g2 = 0 in G1 (64-byte points), 1 in
// G2 (128); all-zero bytes = the identity.  A and every B go through a table first, so that they are loaded under the stored-word
// contract exactly as a widening stage loads them.  Returns 0, -1 for a batch size this was not built for.
}  // extern "C"
static void put_point(HostTab& h, size_t j, const uint8_t* b, int g2) {
  const PtTab t = h.tab();
  if (g2) decode_pool_g2(t, j, b, 0); else decode_pool_g1(t, j, b, 0);
  if (t.st[j] & 0x80) {                       // an identity entry of a table: zero words under the flag, as the builders store it
    static const int32_t zero[BN_LIMBS] = {0};
    for (int e = 0; e < (g2 ? 4 : 2); ++e) put_const(t, e, j, zero);
  }
}
template <class F, int BATCH> static void flow(int g2, const uint8_t* a, const uint8_t* b, uint8_t* out, uint8_t* flags) {
  const size_t sz = g2 ? 128 : 64;
  HostTab src, dst, one;
  src.reset(BATCH, (uint32_t)g2); dst.reset(BATCH, (uint32_t)g2); one.reset(1, (uint32_t)g2);
  put_point(one, 0, a, g2);
  for (int i = 0; i < BATCH; ++i) put_point(src, (size_t)i, b + sz * i, g2);
  Affine<F> A;
  pool_load_aff(one.tab(), 0, A);
  if (A.inf) {                                // as the builders do: the generator's coordinates stand in for an identity A
    Affine<F> gen;
    HostTab gt;
    gt.reset(1, (uint32_t)g2);
    if (g2) decode_pool_g2(gt.tab(), 0, a, 4); else decode_pool_g1(gt.tab(), 0, a, 4);
    pool_load_aff(gt.tab(), 0, gen);
    A.x = gen.x; A.y = gen.y;
  }
  pool_widen_lane<F, BATCH, BATCH>(true, src.tab(), 0, A, dst.tab(), 0);
  g_tab[0] = dst;
  hp_read(0, 0, BATCH, out, flags);
  g_tab[0] = HostTab();
}
extern "C" {
int hp_flow(int g2, int batch, const uint8_t* a, const uint8_t* b, uint8_t* out, uint8_t* flags) {
  if (g2 == 0 && batch == 4) flow<Fp, 4>(0, a, b, out, flags);
  else if (g2 == 0 && batch == 8) flow<Fp, 8>(0, a, b, out, flags);
  else if (g2 == 1 && batch == 4) flow<Fp2, 4>(1, a, b, out, flags);
  else if (g2 == 1 && batch == 8) flow<Fp2, 8>(1, a, b, out, flags);
  else return -1;
  return 0;
}
// non-vacuity of the contract: a sum of two loaded coordinates (|value| up to 2 q, uncarried limbs) stored as it is — under the tracker this
// must abort with a BOUND VIOLATION
void hp_unsafe_store(void) {
  HostTab h;
  h.reset(1, 0);
  const PtTab t = h.tab();
  decode_pool_g1(t, 0, nullptr, 4);
  const Fp x = pt_load_fp(t, 0, 0), y = pt_load_fp(t, 1, 0);
  pt_store_fp(t, 0, 0, fp_add(x, y));
}

}  // extern "C"

#else  // PT_PAIR_CONSUMER

extern "C" {

// The consumer's additions on table records, in the pair layout: acc = rec[0] (the seed: jac_from_affine), then acc += rec[i]
// (jac_accumulate_from) for i = 1 .. n - 1, every record loaded under the stored-word contract (PtRec).  g2 = 0: G1 records of 64 bytes,
// 1: G2 records of 128; all-zero bytes = an identity entry.  out = the affine sum (zeros = the identity).
void hp_consume(int g2, const uint8_t* recs, size_t n, uint8_t* out) {
  HostTab h;
  h.reset(n, (uint32_t)g2);
  const PtTab t = h.tab();
  const size_t sz = g2 ? 128 : 64;
  static const int32_t zero[BN_LIMBS] = {0};
  for (size_t j = 0; j < n; ++j) {
    const uint8_t* b = recs + sz * j;
    const bool inf = all_zero(b, (int)sz);
    for (int e = 0; e < (g2 ? 4 : 2); ++e) { if (inf) put_const(t, e, j, zero); else put_canonical(t, e, j, b + 32 * e); }
    t.st[j] = inf ? 0x80 : 0;
  }
  if (g2) {
    G2Jac acc;
    for (size_t j = 0; j < n; ++j) {
      const PtRec src{t.planes + pt_word(t, 0, j), (t.st[j] & 0x80) != 0};
      if (j == 0) { G2Affine e; src(e); jac_from_affine(acc, e); }
      else jac_accumulate_from(acc, src);
    }
    G2Affine r;
    jac_to_affine(r, acc);
    if (r.inf) { memset(out, 0, 128); return; }
    fp_to_be32(out, r.x.c[0]); fp_to_be32(out + 32, r.x.c[1]); fp_to_be32(out + 64, r.y.c[0]); fp_to_be32(out + 96, r.y.c[1]);
  } else {
    G1Jac acc;
    for (size_t j = 0; j < n; ++j) {
      const PtRec src{t.planes + pt_word(t, 0, j), (t.st[j] & 0x80) != 0};
      if (j == 0) { G1Affine e; src(e); jac_from_affine(acc, e); }
      else jac_accumulate_from(acc, src);
    }
    G1Affine r;
    jac_to_affine(r, acc);
    if (r.inf) { memset(out, 0, 64); return; }
    fp_to_be32(out, r.x); fp_to_be32(out + 32, r.y);
  }
}

}  // extern "C"
#endif
