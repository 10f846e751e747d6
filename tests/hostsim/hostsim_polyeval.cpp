// hostsim_polyeval — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the bodies of the evaluation of polynomials with G2 coefficients (bn254_amd/csrc/bn254_polyeval.h over bn254_dealing.h,
// bn254_threshold.h and bn254_fr.h) — the very functions k_pe_decode, k_pe_eval_lane and k_pe_eval_wave run.  A stand-alone program: it reads
// one command per line from the file named on its command line and answers each with one line, so the same source runs plain, under
// -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated bound) and built with -fsanitize=address,undefined, never loaded into another
// process (tests/test_polyeval_cases.py).
//   eval X MORE_LEN MORE_BITS N {COEFF}*N  -> one polynomial of N coefficients (lowest degree first) at X, the coefficients decoded once:
//                                             "status value status value" (lane layout, wave layout).  The lane walks as in a wave whose
//                                             longest polynomial has N + MORE_LEN coefficients and whose widest x has max(bits of X, MORE_BITS) bits
//   span P M POLY {OFF}*(P+1)              -> "status lo len" of polynomial POLY of P over M coefficients
//   pow X E                                -> X^E mod r as 32 big-endian bytes (the wave layout's chunk scalar)
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
#include "../../bn254_amd/csrc/bn254_polyeval.h"

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

static std::string run(std::istringstream& in) {
  std::string cmd;
  in >> cmd;
  std::ostringstream out;
  if (cmd == "eval") {
    uint32_t x;
    uint64_t more_len;
    int more_bits;
    size_t n;
    in >> x >> more_len >> more_bits >> n;
    // k_pe_decode: exactly n entries, so that a read past the polynomial is a read past the allocation
    std::vector<int32_t> xy(n * PE_COEFF_WORDS);
    std::vector<uint8_t> inf(n), st(n);
    for (size_t s = 0; s < n; ++s) {
      std::string c;
      in >> c;
      Bytes b = unhex(c);
      pe_decode(&xy[s * PE_COEFF_WORDS], inf[s], st[s], b.p());
    }
    uint32_t value[32];
    // k_pe_eval_lane
    {
      G2Jac acc;
      uint8_t est;
      const int bits = pe_bits(x) > more_bits ? pe_bits(x) : more_bits;
      pe_lane_eval(acc, est, x, xy.data(), inf.data(), st.data(), 0, n, n + more_len, bits);
      g2msm_encode((uint8_t*)value, acc, est);
      out << (unsigned)est << " " << hex((const uint8_t*)value, 128);
    }
    // k_pe_eval_wave (the kernel sends the empty polynomial to the lane layout; here it shows that every lane's chunk is then empty)
    {
      std::vector<G2JacSlot> part(BN_CL_WAVE);
      uint32_t cnt[BN_CL_WAVE];
      uint64_t bad[BN_CL_WAVE];
      uint8_t sts[BN_CL_WAVE];
      for (unsigned t = 0; t < BN_CL_WAVE; ++t) {
        G2Jac partial;
        pe_wave_partial(partial, sts[t], bad[t], x, xy.data(), inf.data(), st.data(), 0, n, t);
        pe_wave_scale(part[t].v, partial, x, n, t);
        cnt[t] = 1;
      }
      for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
        for (unsigned t = 0; t < stride; ++t) msm_tree_level(part.data(), cnt, sts, bad, t, stride);
      g2msm_encode((uint8_t*)value, part[0].v, sts[0]);
      out << " " << (unsigned)sts[0] << " " << hex((const uint8_t*)value, 128);
    }
  } else if (cmd == "span") {
    uint64_t p, m, poly;
    in >> p >> m >> poly;
    std::vector<uint64_t> off(p + 1);
    for (auto& o : off) in >> o;
    uint64_t lo;
    uint8_t st;
    const uint64_t len = pe_span(off.data(), p, m, (uint32_t)poly, lo, st);
    out << (unsigned)st << " " << lo << " " << len;
  } else if (cmd == "pow") {
    uint32_t x;
    uint64_t e;
    in >> x >> e;
    uint32_t k[8], be[8];
    pe_chunk_scalar(k, x, e, pe_bits64(e | 1u) + 3);             // a wave's bound is its widest exponent's: leading zero bits change nothing
    u256_to_be((uint8_t*)be, k);
    out << hex((const uint8_t*)be, 32);
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
