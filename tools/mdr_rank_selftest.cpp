// mdr_rank_selftest.cpp -- a stand-alone check of the combination-rank
// arithmetic the MDR kernels run per lane (mdr_binom, mdr_unrank, mdr_next and
// mdr_advance of fs_mdr.h) against a plain enumeration, meant for a sanitizer
// build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude
//       tools/mdr_rank_selftest.cpp -o /tmp/mdr_rank_selftest && /tmp/mdr_rank_selftest
//
// For every p <= 14 and k <= min(6, p): mdr_next from (0, .., k-1) must list
// C(p,k) combinations in itertools.combinations order; mdr_unrank must give
// the listed combination at every rank; mdr_advance from every rank must land
// on the listed combination `step` further, for the steps the kernels take (4
// and 256) and their neighbours.  It includes fs_mdr.h only, links nothing of
// the library and needs no device.  Exit status 0 = every check held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../fastselect_amd/csrc/fs_mdr.h"

using namespace fs;

static long checks = 0;
static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    checks++;                                                            \
    if (!(cond)) {                                                       \
      if (failures < 20)                                                 \
        std::fprintf(stderr, "%s:%d: %s failed (p %d k %d rank %ld step %ld)\n", __FILE__, \
                     __LINE__, #cond, (int)p, k, (long)r, (long)step);   \
      failures++;                                                        \
    }                                                                    \
  } while (0)

// a's successor in lexicographic order, written without fs_mdr.h; false at the last one
static bool plain_next(int p, int k, int32_t* a) {
  int t = k - 1;
  while (t >= 0 && a[t] == p - k + t) t--;
  if (t < 0) return false;
  a[t]++;
  for (int u = t + 1; u < k; u++) a[u] = a[u - 1] + 1;
  return true;
}

int main() {
  const int64_t steps[] = {1, 3, 4, 63, 255, 256, 257, 1000};
  for (int64_t p = 1; p <= 14; p++) {
    for (int k = 1; k <= kMdrMaxK && k <= p; k++) {
      int64_t r = 0, step = 0;
      int64_t count = 0;
      CHECK(mdr_count(p, k, &count));
      // the enumeration, by the plain successor
      std::vector<int32_t> all;
      int32_t a[kMdrMaxK];
      for (int t = 0; t < k; t++) a[t] = t;
      do all.insert(all.end(), a, a + k); while (plain_next((int)p, k, a));
      CHECK((int64_t)all.size() == count * k);
      CHECK((uint64_t)count == mdr_binom(p, k));
      if ((int64_t)all.size() != count * k) continue;
      // mdr_next walks the same list
      int32_t f[kMdrMaxK];
      for (int t = 0; t < k; t++) f[t] = t;
      for (r = 0; r < count; r++) {
        CHECK(std::memcmp(f, &all[(size_t)r * k], (size_t)k * 4) == 0);
        if (r + 1 < count) mdr_next(p, k, f);
      }
      for (r = 0; r < count; r++) {
        int32_t g[kMdrMaxK];
        mdr_unrank(p, k, r, g);
        CHECK(std::memcmp(g, &all[(size_t)r * k], (size_t)k * 4) == 0);
        for (int64_t s : steps) {
          step = s;
          if (r + step >= count) continue;  // mdr_advance's result must exist
          int32_t h[kMdrMaxK];
          std::memcpy(h, g, sizeof(h[0]) * (size_t)k);
          mdr_advance(p, k, h, step);
          CHECK(std::memcmp(h, &all[(size_t)(r + step) * k], (size_t)k * 4) == 0);
        }
        step = 0;
      }
    }
  }
  std::printf("mdr_rank_selftest: %ld checks, %s\n", checks, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
