// mdr_top_selftest.cpp -- a stand-alone check of fs_mdr_scan_top's host-side
// selection (the bounded heaps and their merge, the histogram threshold
// search and the CPU backend around them), meant for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -pthread -Iinclude tools/mdr_top_selftest.cpp \
//       fastselect_amd/csrc/fs_mdr_cpu.cpp -o /tmp/mdr_top_selftest && /tmp/mdr_top_selftest
//
// It links no GPU code and needs no device.  Exit status 0 = every check held.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../fastselect_amd/csrc/fs_mdr.h"

namespace fs {  // what fs_mdr_cpu.cpp takes from the rest of the library
void set_error(const std::string& msg) { std::fprintf(stderr, "error: %s\n", msg.c_str()); }
int hardware_threads(int n_jobs) {
  return n_jobs > 0 ? n_jobs : (int)std::max(1u, std::thread::hardware_concurrency());
}
}  // namespace fs

using namespace fs;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      failures++;                                                        \
    }                                                                    \
  } while (0)

// heap against a full sort, with many equal keys; merge of several heaps
static void check_heaps(std::mt19937& rng) {
  for (size_t n : {(size_t)1, (size_t)7, (size_t)300, (size_t)5000}) {
    std::vector<MdrCand> all;
    for (int64_t r = 0; r < 3000; r++) all.push_back({0x3F000000u + (uint32_t)(rng() % 40), r});
    std::vector<MdrCand> want = all;
    std::sort(want.begin(), want.end(), mdr_cand_before);
    std::shuffle(all.begin(), all.end(), rng);
    std::vector<MdrTopN> part(4, MdrTopN(n));
    for (size_t i = 0; i < all.size(); i++) part[i % 4].push(all[i]);
    MdrTopN m(n);
    for (const MdrTopN& p : part)
      for (const MdrCand& c : p.h) m.push(c);
    const int n_top = (int)n + 3;  // room for padding
    std::vector<float> ba(n_top);
    std::vector<int64_t> rank(n_top);
    m.sorted_into(ba.data(), rank.data(), n_top);
    const size_t have = std::min(n, want.size());
    for (int j = 0; j < n_top; j++) {
      uint32_t bits;
      std::memcpy(&bits, &ba[j], 4);
      if ((size_t)j < have) CHECK(bits == want[j].bits && rank[j] == want[j].rank);
      else CHECK(bits == 0 && rank[j] == -1);
    }
  }
  MdrTopN none(0);
  none.push({1, 1});
  CHECK(none.h.empty());
}

// threshold search against a direct count, and the bin functions' bounds
static void check_threshold(std::mt19937& rng) {
  CHECK(mdr_bin(0) == 0 && mdr_bin(0x3EFFFFFFu) == 0 && mdr_bin(0x3F000000u) == 1);
  CHECK(mdr_bin(0x3F800000u) == (uint32_t)kMdrBins - 1 && mdr_bin(0xFFFFFFFFu) == (uint32_t)kMdrBins - 1);
  for (uint32_t b = 0; b < (uint32_t)kMdrBins; b++) CHECK(mdr_bin(mdr_bin_floor(b)) == b);
  for (uint32_t b = 1; b < (uint32_t)kMdrBins; b++) CHECK(mdr_bin(mdr_bin_floor(b) - 1) == b - 1);
  for (int trial = 0; trial < 200; trial++) {
    std::vector<uint64_t> hist(kMdrBins, 0);
    uint64_t total = 0;
    for (int i = 0; i < 30; i++) {
      const uint64_t c = rng() % 50;
      hist[rng() % kMdrBins] += c;
      total += c;
    }
    if (trial % 3 == 0) hist[0] += 1000, total += 1000;
    if (total == 0) continue;
    const uint64_t need = 1 + rng() % total;
    uint32_t bin;
    uint64_t m;
    mdr_top_threshold(hist.data(), need, &bin, &m);
    uint64_t at = 0, above = 0;
    for (uint32_t b = bin; b < (uint32_t)kMdrBins; b++) at += hist[b];
    for (uint32_t b = bin + 1; b < (uint32_t)kMdrBins; b++) above += hist[b];
    CHECK(m == at && at >= need && above < need);
  }
}

// the CPU backend: 1 thread against 5, entry 0 against fs_mdr_scan, padding
static void check_backend(std::mt19937& rng) {
  const int64_t n = 37, p = 9;
  std::vector<uint8_t> x((size_t)n * p), y((size_t)n);
  std::vector<int32_t> fold((size_t)n);
  for (auto& v : x) v = (uint8_t)(rng() % 3);
  for (int64_t i = 0; i < n; i++) y[i] = (uint8_t)(rng() % 2), fold[i] = (int32_t)(i % 3);
  for (int k : {1, 2, 3}) {
    int64_t count = 0;
    CHECK(mdr_count(p, k, &count));
    for (int n_top : {1, 7, 100}) {
      std::vector<float> b1((size_t)3 * n_top), b5(b1.size()), best(3);
      std::vector<int64_t> r1(b1.size()), r5(b1.size()), best_rank(3);
      CHECK(cpu::mdr_scan_top(x.data(), n, p, y.data(), k, fold.data(), 3, 1, count, n_top,
                              b1.data(), r1.data()) == 0);
      CHECK(cpu::mdr_scan_top(x.data(), n, p, y.data(), k, fold.data(), 3, 5, count, n_top,
                              b5.data(), r5.data()) == 0);
      CHECK(std::memcmp(b1.data(), b5.data(), b1.size() * 4) == 0 && r1 == r5);
      CHECK(cpu::mdr_scan(x.data(), n, p, y.data(), k, fold.data(), 3, 2, count, best.data(),
                          best_rank.data(), nullptr) == 0);
      for (int f = 0; f < 3; f++) {
        CHECK(std::memcmp(&b1[(size_t)f * n_top], &best[f], 4) == 0);
        CHECK(r1[(size_t)f * n_top] == best_rank[f]);
        for (int j = 0; j < n_top; j++)
          CHECK((j < count) == (r1[(size_t)f * n_top + j] >= 0));
      }
    }
  }
}

int main() {
  std::mt19937 rng(12345);
  check_heaps(rng);
  check_threshold(rng);
  check_backend(rng);
  std::printf("mdr_top_selftest: %s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
