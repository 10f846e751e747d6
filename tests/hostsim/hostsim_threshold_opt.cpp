// hostsim_threshold_opt — TEST INFRASTRUCTURE ONLY.
//
// Host compilation of the bookkeeping of the optimistic threshold call (bn254_amd/csrc/bn254_threshold.h: tho_candidate, tho_settle,
// tho_gate, tho_reclaims, tho_resettle over bn254_collect.h's flags) — the very functions k_tho_rows, k_tho_settle and k_tho_resettle run,
// in the order th_combine_opt_device enqueues them.  A stand-alone program like hostsim_threshold.cpp: one command per line of the file
// named on its command line, one line of answer each; built plain, under -DBN_TRACK_BOUNDS and with -fsanitize=address,undefined, never
// loaded into another process (tests/test_threshold_opt_cases.py).
//   opt W T TUPLE_ST VERDICT NSH {KEY PRE EXACT}*NSH
//     one tuple of NSH shares over rows of W words, threshold T: TUPLE_ST its status behind the range rule and the hash, PRE a share's
//     pre-check status, EXACT the status the exact verify would give it, VERDICT what the tuple check says if it is asked.  Answer:
//     "flag gate count row.. zeroed | exact gate tuple_st count row.. zeroed" — the first half behind the candidate rows and tho_settle, the
//     second behind the verdict, the queue's verify, the second claim pass and tho_resettle; zeroed = 1 iff the stage zeroed the signature.
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

static bool zeroed(const uint32_t* sig) {
  for (int k = 0; k < 16; ++k) if (sig[k]) return false;
  return true;
}
static void mark(uint32_t* sig) { for (int k = 0; k < 16; ++k) sig[k] = 0xA5A5A5A5u; }

static std::string run(std::istringstream& in) {
  std::string cmd;
  in >> cmd;
  std::ostringstream out;
  if (cmd != "opt") return "?";
  size_t w, nsh;
  uint32_t t;
  unsigned tuple_in, verdict_in;
  in >> w >> t >> tuple_in >> verdict_in >> nsh;
  // exactly the sizes the call has: a row of w words, nsh shares (the sanitised build sees any step past them)
  std::vector<uint32_t> key(nsh), row(w, 0);
  std::vector<uint8_t> pre(nsh), exact(nsh), share_st(nsh);
  for (size_t s = 0; s < nsh; ++s) {
    unsigned a, b;
    in >> key[s] >> a >> b;
    pre[s] = (uint8_t)a; exact[s] = (uint8_t)b;
  }
  const size_t n = 1;
  uint8_t tuple_st[1] = {(uint8_t)tuple_in}, dup[1] = {0}, flag[1], verdict[1] = {(uint8_t)verdict_in}, gate[1];
  uint32_t sig[16], count = 0xFFFFFFFFu;
  // the candidate rows (k_tho_rows, first pass): only the shares of an accepted tuple are looked at; a tuple whose status is non-zero has
  // no candidate (the pre-check gave its shares the hash status, or they are nobody's)
  for (size_t s = 0; s < nsh; ++s) {
    share_st[s] = pre[s];
    if (share_st[s] == ST_OK) tho_candidate(row.data(), w, key[s], &dup[0]);
  }
  mark(sig);
  flag[0] = tho_settle(row.data(), w, t, tuple_st[0], dup[0], (uint8_t*)sig, count);
  gate[0] = tho_gate(flag[0]);
  out << (unsigned)flag[0] << " " << (unsigned)gate[0] << " " << count;
  for (size_t k = 0; k < w; ++k) out << " " << std::hex << row[k] << std::dec;
  out << " " << (zeroed(sig) ? 1 : 0) << " |";
  // behind the tuple check: k_clo_settle zeroes the row of a tuple that goes the exact way, the queue's verify gives its candidates their
  // exact statuses, the second claim pass and tho_resettle
  const bool goes = clo_goes_exact(flag[0], verdict[0]);
  if (goes)
    for (size_t k = 0; k < w; ++k) row[k] = 0;
  for (size_t s = 0; s < nsh; ++s)
    if (clo_queued(share_st[s], 0, n, flag, verdict)) share_st[s] = exact[s];
  uint8_t ignored = 0;
  for (size_t s = 0; s < nsh; ++s)
    if (tho_reclaims(share_st[s], 0, n, flag, verdict)) tho_candidate(row.data(), w, key[s], &ignored);
  mark(sig);
  bool mine = false;
  uint8_t st = tuple_st[0];
  uint32_t count2 = count;
  gate[0] = tho_resettle(row.data(), w, t, flag[0], verdict[0], st, (uint8_t*)sig, count2, mine);
  if (mine) { tuple_st[0] = st; count = count2; }
  out << " " << (goes ? 1 : 0) << " " << (unsigned)gate[0] << " " << (unsigned)tuple_st[0] << " " << count;
  for (size_t k = 0; k < w; ++k) out << " " << std::hex << row[k] << std::dec;
  out << " " << (zeroed(sig) ? 1 : 0);
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
