// hostsim_reshare — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the bodies of the vector combine and of the reshare (bn254_amd/csrc/bn254_reshare.h over bn254_polyeval.h,
// bn254_dealing.h, bn254_threshold.h and bn254_fr.h) — the very functions k_pe_decode, k_vc_term, k_rs_qualify, k_rs_select, k_rs_coeff and the
// two segment sums run, under a loop over lanes.  A stand-alone program: it reads one command per line from the file named on its command
// line and answers each with one line, so the same source runs plain, under -DBN_TRACK_BOUNDS (the interval tracker aborts on a violated
// bound) and built with -fsanitize=address,undefined, never loaded into another process (tests/test_reshare_cases.py).
//   vc REDUCE D LEN {SCALAR}*D {POINT}*(D*LEN)      -> "st value" per column in the lane layout of the sums, then the same in the wave layout
//   rs N T LEN D BMW {KEYST KEY}*N {DKEY}*D {POINT}*(D*LEN)
//                                                   -> "status |Q| {dealer_st}*D {row word}*BMW" and, when the status is 0, "{pick}*T {lambda}*T";
//                                                      then the commitments as vc prints its columns (zero bytes behind a raised stop byte)
// Points are vector-major, 128 bytes as hex; scalars 32 bytes as hex; a registered key is its registration status and its bytes.
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
#include "../../bn254_amd/csrc/bn254_reshare.h"

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

// the decoded points of a call: exactly `count` entries, so that a read past the end is a read past the allocation
struct Decoded {
  std::vector<int32_t> xy;
  std::vector<uint8_t> inf, st;
  void read(std::istringstream& in, size_t count) {
    xy.resize(count * PE_COEFF_WORDS), inf.resize(count), st.resize(count);
    for (size_t s = 0; s < count; ++s) {
      std::string c;
      in >> c;
      Bytes b = unhex(c);
      pe_decode(&xy[s * PE_COEFF_WORDS], inf[s], st[s], b.p());
    }
  }
};

// k_vc_term over every lane of its grid (whole waves: the lanes past the end walk too), then the two sums of every column; `stop`: the
// raised stop byte — no term, zero bytes
static void terms_and_sums(std::ostringstream& out, const Decoded& pts, const uint8_t* scalars, const uint32_t* pick, uint64_t T, uint64_t len, bool reduce, bool stop) {
  const uint64_t m = stop ? 0 : T * len;
  std::vector<G2Jac> terms(m);
  std::vector<uint8_t> term_st(m);
  for (uint64_t s = 0; s < (m + 63) / 64 * 64; ++s) {
    G2Jac t;
    uint8_t st;
    vc_term(t, st, pts.xy.data(), pts.inf.data(), pts.st.data(), scalars, pick, T, len, s, reduce, s < m);
    if (s < m) { terms[s] = t; term_st[s] = st; }
  }
  std::vector<uint64_t> seg(len + 1);
  for (uint64_t k = 0; k <= len; ++k) seg[k] = k * T;
  uint32_t value[32];
  for (int layout = 0; layout < 2; ++layout)
    for (uint64_t k = 0; k < len; ++k) {
      if (stop) { out << " 0 " << std::string(256, '0'); continue; }
      uint8_t seg_st;
      const uint64_t n = msm_seg_len(seg.data(), k, m, nullptr, seg_st);
      uint8_t st = ST_OK;
      if (layout == 0) {                                      // k_g2msm_sum_lane
        G2Jac acc;
        msm_lane_sum(acc, st, terms.data(), term_st.data(), n ? seg[k] : 0, n);
        if (seg_st != ST_OK) st = seg_st;
        g2msm_encode((uint8_t*)value, acc, st);
      } else {                                                // k_g2msm_sum_wave
        std::vector<G2JacSlot> part(BN_CL_WAVE);
        uint32_t cnt[BN_CL_WAVE];
        uint64_t bad[BN_CL_WAVE];
        uint8_t sts[BN_CL_WAVE];
        for (unsigned t = 0; t < BN_CL_WAVE; ++t) {
          msm_wave_partial(part[t].v, sts[t], bad[t], terms.data(), term_st.data(), seg[k], n, t);
          cnt[t] = 1;
        }
        for (unsigned stride = BN_CL_WAVE / 2; stride >= 1; stride >>= 1)
          for (unsigned t = 0; t < stride; ++t) msm_tree_level(part.data(), cnt, sts, bad, t, stride);
        st = sts[0];
        g2msm_encode((uint8_t*)value, part[0].v, st);
      }
      out << " " << (unsigned)st << " " << hex((const uint8_t*)value, 128);
    }
}

static std::string run(std::istringstream& in) {
  std::string cmd;
  in >> cmd;
  std::ostringstream out;
  if (cmd == "vc") {
    int reduce;
    uint64_t d, len;
    in >> reduce >> d >> len;
    std::vector<uint32_t> scalars(8 * d + 1);
    for (uint64_t i = 0; i < d; ++i) {
      std::string c;
      in >> c;
      Bytes b = unhex(c);
      memcpy(&scalars[8 * i], b.p(), 32);
    }
    Decoded pts;
    pts.read(in, d * len);
    out << "vc";
    terms_and_sums(out, pts, (const uint8_t*)scalars.data(), nullptr, d, len, reduce != 0, false);
  } else if (cmd == "rs") {
    uint64_t n, len, d, bmw;
    uint32_t t;
    in >> n >> t >> len >> d >> bmw;
    std::vector<uint8_t> key_st(n);
    Decoded keys;
    keys.xy.resize(n * PE_COEFF_WORDS), keys.inf.resize(n), keys.st.resize(n);
    for (uint64_t j = 0; j < n; ++j) {
      unsigned st;
      std::string c;
      in >> st >> c;
      Bytes b = unhex(c);
      pe_decode(&keys.xy[j * PE_COEFF_WORDS], keys.inf[j], keys.st[j], b.p());   // a refused key lies in the table under the generator's coordinates
      key_st[j] = (uint8_t)st;
    }
    std::vector<uint32_t> dealer_key(d);
    for (auto& k : dealer_key) in >> k;
    Decoded pts;
    pts.read(in, d * len);
    // k_rs_qualify
    std::vector<uint8_t> dealer_st(d);
    for (uint64_t i = 0; i < d; ++i)
      dealer_st[i] = rs_qualify(pts.xy.data(), pts.inf.data(), pts.st.data(), len, dealer_key.data(), i, keys.xy.data(), key_st.data(), keys.inf.data(), n);
    // k_rs_select
    std::vector<uint32_t> pick(d), row(bmw, 0);
    uint32_t part[BN_CL_WAVE];
    for (unsigned l = 0; l < BN_CL_WAVE; ++l) part[l] = rs_count(dealer_st.data(), d, l);
    const uint32_t total = rs_prefix(part);
    uint8_t skip, status;
    rs_verdict(skip, status, total, t);
    for (unsigned l = 0; l < BN_CL_WAVE; ++l) rs_select_lane(pick.data(), row.data(), bmw, dealer_key.data(), dealer_st.data(), d, l, part[l], total, t);
    out << (unsigned)status << " " << total;
    for (uint64_t i = 0; i < d; ++i) out << " " << (unsigned)dealer_st[i];
    for (uint64_t w = 0; w < bmw; ++w) out << " " << row[w];
    // k_rs_coeff
    std::vector<uint32_t> scalars(8 * d + 1, 0xEEEEEEEEu);
    if (!skip) {
      for (uint64_t r = 0; r < t; ++r) rs_coeff((uint8_t*)scalars.data(), pick.data(), dealer_key.data(), row.data(), bmw, r);
      for (uint64_t r = 0; r < t; ++r) out << " " << pick[r];
      for (uint64_t r = 0; r < t; ++r) out << " " << hex((const uint8_t*)&scalars[8 * pick[r]], 32);
    }
    terms_and_sums(out, pts, (const uint8_t*)scalars.data(), pick.data(), t, len, false, skip != 0);
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
