// Host compilation of the proof-of-possession front end (bn254_amd/csrc/bn254_pop.h: the composer of the messages TAG || pk and the fold of two
// status arrays) — test infrastructure only (tests/test_pop_msgs.py).  Every function walks the elements the device launch would: the grid
// of k_pop_compose / k_pop_fold rounded up to whole workgroups of HP_WG lanes, so the lanes past the last element run too and must write
// nothing.  With -DHP_MAIN the file is a stand-alone program for the sanitizers: exact-size heap buffers, results checked against a direct
// restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../bn254_amd/csrc/bn254_pop.h"

using namespace bn254;

#define HP_WG 256   /* POP_WG of bn254_pop.hip */
static size_t hp_grid_lanes(size_t elems) { return (elems + HP_WG - 1) / HP_WG * HP_WG; }

extern "C" {

int hp_msg_bytes(void) { return BN_POP_MSG_BYTES; }
const char* hp_tag(void) { return BN254_POP_TAG; }
// the launch of k_pop_compose over n keys; key_idx may be null (the prove and verify calls)
void hp_compose(const uint8_t* pks, size_t n, uint8_t* msgs, uint64_t* off, uint32_t* key_idx) {
  const PopMsgs out = {(uint32_t*)msgs, off, key_idx};
  const size_t lanes = hp_grid_lanes(pop_compose_elems(n));
  for (size_t t = 0; t < lanes; ++t) pop_compose_elem(t, n, (const uint32_t*)pks, out);
}
// the launch of k_pop_fold over n statuses
void hp_fold(size_t n, uint8_t* first, const uint8_t* second) {
  const size_t lanes = hp_grid_lanes(n);
  for (size_t j = 0; j < lanes; ++j) pop_fold_elem(j, n, first, second);
}
int hp_fold_one(int first, int second) { return pop_fold((uint8_t)first, (uint8_t)second); }

}  // extern "C"

#ifdef HP_MAIN
static int hp_check(size_t n, bool with_idx) {
  // exact sizes: a byte written past 144 n, offset n + 1 or index n is a heap overflow the sanitizer reports (n = 0: malloc(0) blocks)
  uint8_t* pks = (uint8_t*)malloc(128 * n);
  uint8_t* msgs = (uint8_t*)malloc((size_t)BN_POP_MSG_BYTES * n);
  uint64_t* off = (uint64_t*)malloc(sizeof(uint64_t) * (n + 1));
  uint32_t* idx = with_idx ? (uint32_t*)malloc(sizeof(uint32_t) * n) : nullptr;
  for (size_t i = 0; i < 128 * n; ++i) pks[i] = (uint8_t)(i * 131 + 7 * (i >> 7) + 1);
  hp_compose(pks, n, msgs, off, idx);
  int bad = 0;
  for (size_t j = 0; j < n; ++j) {
    bad |= memcmp(msgs + 144 * j, BN254_POP_TAG, 16) != 0;
    bad |= memcmp(msgs + 144 * j + 16, pks + 128 * j, 128) != 0;
    bad |= with_idx && idx[j] != j;
  }
  for (size_t j = 0; j <= n; ++j) bad |= off[j] != 144 * j;
  uint8_t* a = (uint8_t*)malloc(n);
  uint8_t* b = (uint8_t*)malloc(n);
  for (size_t j = 0; j < n; ++j) { a[j] = (uint8_t)(j % 12); b[j] = (uint8_t)(j / 12 % 12); }
  hp_fold(n, a, b);
  for (size_t j = 0; j < n; ++j) bad |= a[j] != (j % 12 ? j % 12 : j / 12 % 12);
  free(pks); free(msgs); free(off); free(idx); free(a); free(b);
  return bad;
}
int main() {
  const size_t sizes[] = {0, 1, 2, 7, 8, 63, 64, 65, 130, 144, 257};
  int bad = 0;
  for (size_t n : sizes) bad |= hp_check(n, true) | hp_check(n, false);
  for (int a = 0; a < 12; ++a) for (int b = 0; b < 12; ++b) bad |= hp_fold_one(a, b) != (a ? a : b);
  if (bad) { printf("hostsim_pop FAILED\n"); return 1; }
  printf("hostsim_pop ok\n");
  return 0;
}
#endif
