// hostsim_dealing — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the bodies of the G2 weighted sum and of the dealing check (bn254_amd/csrc/bn254_dealing.h over bn254_threshold.h and
// bn254_fr.h) — the very functions k_g2msm_term, k_g2msm_sum_lane, k_g2msm_sum_wave, k_dl_scan, k_dl_fact, k_dl_tables, k_dl_coeff and
// k_dl_settle run.  A stand-alone program: it reads one command per line from the file named on its command line and answers each with one
// line, so the same source runs plain, under -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated bound) and built with
// -fsanitize=address,undefined, never loaded into another process (tests/test_dealing_cases.py).
//   coef N T SEED                          -> "c_0 .. c_N-1 l_0 .. l_T-1": the check's coefficients and the Lagrange coefficients of the points 1 .. T
//   msm REDUCE M {POINT SCALAR}*M          -> one segment of the weighted sum, the terms computed once: "status sum status sum" (lane layout, wave layout)
//   check LAYOUT T SEED N {KEY ST}*N       -> the whole call over a key table built as registration builds it, registration statuses given:
//                                             "status bad_key group_pk"; LAYOUT 0 lane, 1 wave
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#if defined(BN_TRACK_BOUNDS)
#include "../../bn254_amd/csrc/bn254_norm_sites.h"
extern "C" { signed char bn_site_mode[1024]; unsigned int bn_site_hits[1024]; signed char bn_site_dflt[1024]; int bn_bound_soft = 0; int bn_bound_failed = 0; }
static struct BnSiteInit { BnSiteInit() { for (int i = 0; i < 1024; ++i) bn_site_mode[i] = (signed char)bn_site_override(i); } } bn_site_init_;
#endif

#include "../../bn254_amd/csrc/bn254_hash.h"
#include "../../bn254_amd/csrc/bn254_io.h"
#include "../../bn254_amd/csrc/bn254_pairing.h"
#include "../../bn254_amd/csrc/bn254_collect.h"
#include "../../bn254_amd/csrc/bn254_fr.h"
#include "../../bn254_amd/csrc/bn254_threshold.h"
#include "../../bn254_amd/csrc/bn254_dealing.h"

using namespace bn254;

// aligned byte buffers: the decoders read 32-bit words
struct Bytes {
  std::vector<uint32_t> w;
  size_t len = 0;
  uint8_t* p() { return (uint8_t*)w.data(); }
};
static Bytes unhex(const std::string& s) {
  Bytes b;
  b.len = s.size() / 2;
  b.w.assign(b.len / 4 + 1, 0);
  for (size_t i = 0; i < b.len; ++i) b.p()[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
  return b;
}
static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return s;
}
static void seed_words(uint32_t* w, const std::string& seed_hex) {
  Bytes b = unhex(seed_hex);
  for (int j = 0; j < 8; ++j)
    w[j] = ((uint32_t)b.p()[4 * j] << 24) | ((uint32_t)b.p()[4 * j + 1] << 16) | ((uint32_t)b.p()[4 * j + 2] << 8) | b.p()[4 * j + 3];
}

// the sum of one segment of `len` terms from `lo` in either layout, as the kernels run it
static void sum_segment(int layout, const G2Jac* terms, const uint8_t* term_st, uint64_t lo, uint64_t len, G2Jac& acc, uint8_t& st) {
  st = ST_OK;
  if (layout == 0) { msm_lane_sum(acc, st, terms, term_st, lo, len); return; }
  std::vector<G2JacSlot> part(BN_CL_WAVE);
  uint32_t cnt[BN_CL_WAVE];
  uint64_t bad[BN_CL_WAVE];
  uint8_t sts[BN_CL_WAVE];
  for (unsigned t = 0; t < BN_CL_WAVE; ++t) { msm_wave_partial(part[t].v, sts[t], bad[t], terms, term_st, lo, len, t); cnt[t] = 1; }
  for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
    for (unsigned t = 0; t < stride; ++t) msm_tree_level(part.data(), cnt, sts, bad, t, stride);
  acc = part[0].v;
  st = sts[0];
}
// the three coefficient kernels, lane by lane: scalars = lambda_0 .. lambda_t-1, c_0 .. c_n-1 (32 B each)
static void coefficients(std::vector<uint32_t>& scalars, uint32_t n, uint32_t t, const uint32_t* seed) {
  std::vector<Fr> fact(n + 1), inv(n + 1), w(n - t + 1);
  Fr part[BN_CL_WAVE];
  for (unsigned l = 0; l < BN_CL_WAVE; ++l) part[l] = dl_fact_partial(n + 1, l);
  dl_fact_prefix(part);
  for (unsigned l = 0; l < BN_CL_WAVE; ++l) dl_fact_write(fact.data(), n + 1, l, part[l]);
  scalars.assign(8 * ((size_t)t + n) + 1, 0);
  uint8_t* sc = (uint8_t*)scalars.data();
  for (uint32_t m = 0; m <= n; ++m) dl_tables(inv.data(), w.data(), sc + 32 * (size_t)t, fact.data(), seed, n, t, m);
  for (uint32_t k = 0; k < t; ++k) {
    Fr lambda, ck;
    dl_coeff(lambda, ck, fact.data(), inv.data(), w.data(), n, t, k);
    fr_to_be(sc + 32 * (size_t)k, lambda);
    fr_to_be(sc + 32 * ((size_t)t + k), ck);
  }
}

static std::string run(std::istringstream& in) {
  std::string cmd;
  in >> cmd;
  std::ostringstream out;
  if (cmd == "coef") {
    uint32_t n, t;
    std::string seed_hex;
    in >> n >> t >> seed_hex;
    uint32_t seed[8];
    seed_words(seed, seed_hex);
    std::vector<uint32_t> scalars;
    coefficients(scalars, n, t, seed);
    const uint8_t* sc = (const uint8_t*)scalars.data();
    for (uint32_t j = 0; j < n; ++j) out << (j ? " " : "") << hex(sc + 32 * ((size_t)t + j), 32);
    for (uint32_t k = 0; k < t; ++k) out << " " << hex(sc + 32 * (size_t)k, 32);
  } else if (cmd == "msm") {
    int reduce;
    size_t m;
    in >> reduce >> m;
    std::vector<G2Jac> terms(m + 1);
    std::vector<uint8_t> term_st(m + 1);
    for (size_t s = 0; s < m; ++s) {
      std::string p, k;
      in >> p >> k;
      Bytes bp = unhex(p), bk = unhex(k);
      g2msm_term(terms[s], term_st[s], bp.p(), bk.p(), reduce != 0, true);
    }
    const uint64_t seg[2] = {0, m};
    uint8_t seg_st;
    const uint64_t len = msm_seg_len(seg, 0, m, nullptr, seg_st);
    for (int layout = 0; layout < 2; ++layout) {
      G2Jac acc;
      uint8_t st;
      sum_segment(layout, terms.data(), term_st.data(), 0, len, acc, st);
      uint32_t sum[32];
      g2msm_encode((uint8_t*)sum, acc, st);
      out << (layout ? " " : "") << (unsigned)st << " " << hex((const uint8_t*)sum, 128);
    }
  } else if (cmd == "check") {
    int layout;
    uint32_t t, n;
    std::string seed_hex;
    in >> layout >> t >> seed_hex >> n;
    uint32_t seed[8];
    seed_words(seed, seed_hex);
    // the table as k_register_keys leaves it: a key that does not decode, or the identity, under the generator's coordinates
    std::vector<int32_t> key_xy((size_t)n * 4 * BN_LIMBS + 1);
    std::vector<uint8_t> key_st(n + 1), key_inf(n + 1);
    for (uint32_t j = 0; j < n; ++j) {
      std::string p;
      unsigned st;
      in >> p >> st;
      Bytes b = unhex(p);
      G2Affine q;
      const uint8_t dec = decode_g2(q, b.p(), 0);
      if (dec != ST_OK || q.inf) { q.x = fp2_load_const(C_G2_GEN[0]); q.y = fp2_load_const(C_G2_GEN[1]); }
      if (dec != ST_OK) q.inf = false;
      const Fp xy[4] = {q.x.c0, q.x.c1, q.y.c0, q.y.c1};
      for (int e = 0; e < 4; ++e)
        for (int k = 0; k < BN_LIMBS; ++k) key_xy[((size_t)j * 4 + e) * BN_LIMBS + k] = xy[e].v[k];
      key_st[j] = (uint8_t)st;
      key_inf[j] = q.inf;
    }
    // k_dl_scan
    uint32_t bad_key = UINT32_MAX;
    uint8_t bad_st = ST_OK;
    for (unsigned l = 0; l < BN_CL_WAVE; ++l) {
      uint32_t k;
      uint8_t s;
      dl_scan_lane(k, s, key_st.data(), n, l);
      dl_scan_fold(bad_key, bad_st, k, s);
    }
    const bool t_over = t > n;
    const uint8_t stop = (bad_key != UINT32_MAX || t_over) ? MSM_SEG_MASKED : 0;
    const uint8_t gate[2] = {stop, stop};
    uint32_t sums[64];
    for (int k = 0; k < 64; ++k) sums[k] = 0xA5A5A5A5u;
    uint8_t sum_st[2] = {0xA5, 0xA5};
    if (!stop) {
      const uint32_t n_check = t < n ? n : 0;
      const size_t m = (size_t)t + n_check;
      std::vector<uint32_t> scalars;
      coefficients(scalars, n, t, seed);
      const uint8_t* sc = (const uint8_t*)scalars.data();
      std::vector<G2Jac> terms(m + 1);
      std::vector<uint8_t> term_st(m + 1, ST_OK);
      for (size_t s = 0; s < m; ++s) {
        const size_t key = s < t ? s : s - t;
        g2msm_term_key(terms[s], &key_xy[key * 4 * BN_LIMBS], key_inf[key] != 0, sc + 32 * s, true);
      }
      const uint64_t seg[3] = {0, t, m};
      for (size_t i = 0; i < 2; ++i) {
        uint8_t seg_st;
        const uint64_t len = msm_seg_len(seg, i, m, gate, seg_st);
        G2Jac acc;
        sum_segment(layout, terms.data(), term_st.data(), seg[i], len, acc, sum_st[i]);
        g2msm_encode((uint8_t*)&sums[32 * i], acc, sum_st[i]);
      }
    }
    DlResult r;
    dl_settle(r, bad_key, bad_st, t_over, (const uint8_t*)sums, sum_st);
    out << (unsigned)r.status << " " << r.bad_key << " " << hex(r.pk, 128);
  } else {
    out << "?";
  }
  return out.str();
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s COMMANDS\n", argv[0]); return 2; }
  std::ifstream f(argv[1]);
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::cout << run(in) << "\n";
  }
  return 0;
}
