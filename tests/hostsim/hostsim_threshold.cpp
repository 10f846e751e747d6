// hostsim_threshold — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of Fr (bn254_amd/csrc/bn254_fr.h) and of the rank / select / coefficient / term / sum bodies of the threshold call and
// the scalar-weighted sum (bn254_amd/csrc/bn254_threshold.h) — the very functions k_th_settle, k_th_coeff, k_msm_term, k_msm_sum_lane and
// k_msm_sum_wave run.  A stand-alone program: it reads one command per line from the file named on its command line and answers each with
// one line of hex, so the same source runs plain, under -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated bound) and built with
// -fsanitize=address,undefined, never loaded into another process (tests/test_threshold_cases.py).
//   fr OP A B                      -> the Fr hook's op (0 mul 1 add 2 sub 3 neg 4 inv 5 round trip 6 the uint32 load of A's low word) on 32-byte big-endian operands
//   lag M X0 .. XM-1               -> the M Lagrange coefficients at zero of the points (decimal uint32)
//   trim W T ROW0 .. ROWW-1        -> the row (hex words) cut down to its T lowest bits
//   comb LAYOUT W T NSH {POINT KEY ST}*NSH -> one tuple behind the collect: statuses given; the claim pass, settle, coefficients, terms and
//                                     the sum in layout 0 (lane) / 1 (wave): "tuple_st count row.. used.. sig"
//   msm LAYOUT REDUCE M {POINT SCALAR}*M   -> one segment of the weighted sum: "status sum"
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

#include "../../bn254_amd/csrc/bn254_io.h"
#include "../../bn254_amd/csrc/bn254_pairing.h"
#include "../../bn254_amd/csrc/bn254_collect.h"
#include "../../bn254_amd/csrc/bn254_fr.h"
#include "../../bn254_amd/csrc/bn254_threshold.h"

using namespace bn254;

struct Slot { G1Jac v; int32_t pad; };

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
static std::string fr_hex(const Fr& a) {
  uint32_t out[8];
  fr_to_be((uint8_t*)out, a);
  return hex((const uint8_t*)out, 32);
}

// the sum of one segment of `len` terms from `lo` in either layout, as the kernels run it
static void sum_segment(int layout, const G1Jac* terms, const uint8_t* term_st, uint64_t lo, uint64_t len, G1Jac& acc, uint8_t& st) {
  st = ST_OK;
  if (layout == 0) { msm_lane_sum(acc, st, terms, term_st, lo, len); return; }
  std::vector<Slot> part(BN_CL_WAVE);
  uint32_t cnt[BN_CL_WAVE];
  uint64_t bad[BN_CL_WAVE];
  uint8_t sts[BN_CL_WAVE];
  for (unsigned t = 0; t < BN_CL_WAVE; ++t) { msm_wave_partial(part[t].v, sts[t], bad[t], terms, term_st, lo, len, t); cnt[t] = 1; }
  for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
    for (unsigned t = 0; t < stride; ++t) msm_tree_level(part.data(), cnt, sts, bad, t, stride);
  acc = part[0].v;
  st = sts[0];
}

static std::string run(std::istringstream& in) {
  std::string cmd;
  in >> cmd;
  std::ostringstream out;
  if (cmd == "fr") {
    int op;
    std::string a, b;
    in >> op >> a >> b;
    Bytes ba = unhex(a), bb = unhex(b);
    const Fr x = fr_from_be(ba.p()), y = fr_from_be(bb.p());
    Fr r;
    switch (op) {
      case 0: r = fr_mul(x, y); break;
      case 1: r = fr_add(x, y); break;
      case 2: r = fr_sub(x, y); break;
      case 3: r = fr_neg(x); break;
      case 4: r = fr_inv(x); break;
      case 6: r = fr_from_u32(__builtin_bswap32(((const uint32_t*)ba.p())[7])); break;
      default: r = x; break;
    }
    out << fr_hex(r);
  } else if (cmd == "lag") {
    size_t m;
    in >> m;
    std::vector<uint32_t> x(m + 1);
    for (size_t k = 0; k < m; ++k) in >> x[k];
    for (size_t j = 0; j < m; ++j) out << (j ? " " : "") << fr_hex(th_lagrange_points(x.data(), m, j));
  } else if (cmd == "trim") {
    size_t w;
    uint32_t t;
    in >> w >> t;
    std::vector<uint32_t> row(w + 1);
    for (size_t k = 0; k < w; ++k) in >> std::hex >> row[k] >> std::dec;
    th_trim(row.data(), w, t);
    for (size_t k = 0; k < w; ++k) out << (k ? " " : "") << std::hex << row[k] << std::dec;
  } else if (cmd == "comb") {
    int layout;
    size_t w, nsh;
    uint32_t t;
    in >> layout >> w >> t >> nsh;
    std::vector<uint32_t> shares(16 * nsh + 1), keys(nsh + 1);
    std::vector<uint8_t> share_st(nsh + 1);
    for (size_t s = 0; s < nsh; ++s) {
      std::string p;
      unsigned st;
      in >> p >> keys[s] >> st;
      Bytes b = unhex(p);
      memcpy(&shares[16 * s], b.p(), 64);
      share_st[s] = (uint8_t)st;
    }
    const uint64_t off[2] = {0, nsh};
    uint8_t tuple_st[1] = {ST_OK};
    const ClShares cin = {(const uint8_t*)shares.data(), keys.data(), off, share_st.data(), tuple_st};
    // the collect's claim pass (row V; its sum is overwritten), then this call's steps
    std::vector<uint32_t> row(w + 1, 0), claim(w + 1, 0);
    { G1Jac acc; uint32_t count; cl_lane_sum(acc, count, row.data(), w, cin, 0, nsh); }
    uint32_t sig[16];
    for (int k = 0; k < 16; ++k) sig[k] = 0xA5A5A5A5u;
    const uint32_t count = th_settle(row.data(), w, t, tuple_st[0], (uint8_t*)sig);
    const uint64_t end[1] = {nsh};
    std::vector<G1Jac> terms(nsh + 1);
    std::vector<uint8_t> term_st(nsh + 1);
    for (size_t s = 0; s < nsh; ++s) {
      const size_t tup = cl_tuple_of(s, end, off, 1);
      const bool take = th_take(cin, s, tup, 1, row.data(), claim.data(), w);
      uint32_t k32[8] = {0};
      if (take) fr_to_be((uint8_t*)k32, th_lagrange_row(row.data(), w, keys[s]));
      // as k_msm_term with a wave of one lane: nobody to take, no ladder (layout 0 walks it all the same: the masked-out lane's path)
      if (take || layout == 0) msm_term(terms[s], term_st[s], (const uint8_t*)&shares[16 * s], (const uint8_t*)k32, false, take);
      else { jac_set_identity(terms[s]); term_st[s] = ST_OK; }
    }
    uint8_t seg_st;
    const uint64_t len = msm_seg_len(off, 0, nsh, tuple_st, seg_st);
    if (seg_st != MSM_SEG_MASKED) {
      G1Jac acc;
      uint8_t st;
      sum_segment(layout, terms.data(), term_st.data(), 0, len, acc, st);
      msm_encode((uint8_t*)sig, acc, st);
    }
    out << (unsigned)tuple_st[0] << " " << count;
    for (size_t k = 0; k < w; ++k) out << " " << std::hex << row[k] << std::dec;
    for (size_t k = 0; k < w; ++k) out << " " << std::hex << claim[k] << std::dec;
    out << " " << hex((const uint8_t*)sig, 64);
  } else if (cmd == "msm") {
    int layout, reduce;
    size_t m;
    in >> layout >> reduce >> m;
    std::vector<G1Jac> terms(m + 1);
    std::vector<uint8_t> term_st(m + 1);
    for (size_t s = 0; s < m; ++s) {
      std::string p, k;
      in >> p >> k;
      Bytes bp = unhex(p), bk = unhex(k);
      msm_term(terms[s], term_st[s], bp.p(), bk.p(), reduce != 0, true);
    }
    const uint64_t seg[2] = {0, m};
    uint8_t seg_st;
    const uint64_t len = msm_seg_len(seg, 0, m, nullptr, seg_st);
    G1Jac acc;
    uint8_t st;
    sum_segment(layout, terms.data(), term_st.data(), 0, len, acc, st);
    uint32_t sig[16];
    msm_encode((uint8_t*)sig, acc, st);
    out << (unsigned)st << " " << hex((const uint8_t*)sig, 64);
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
