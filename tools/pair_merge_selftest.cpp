// pair_merge_selftest.cpp -- a stand-alone check of the host side of the pair
// screen's selection (fs_pairscan.h): the ordered key of a score, the total
// order, the pair rank arithmetic, and the bounded list PairTopN with its
// threshold, against a plain sort; meant for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude
//       tools/pair_merge_selftest.cpp -o /tmp/pair_merge_selftest && /tmp/pair_merge_selftest
//
// * pair_key: over a ladder of doubles (negative, subnormal, both zeros,
//   infinities) a < b <=> key(a) < key(b) and a == b <=> equal keys, so -0.0 and
//   +0.0 share a key; pair_score(pair_key(v)) == v, +0.0 for either zero; no
//   key is kPairNoKey.
// * pair_rank / pair_unrank: every pair of every p <= 70 in
//   itertools.combinations order, and the ends of the range at large p.
// * PairTopN: streams of random keys, of masses of equal keys (few distinct
//   scores, zeros of both signs, negative scores), pushed in launch-sized
//   batches with the GPU backend's protocol -- a batch holds only what beats
//   the threshold the list gave before the batch, then compact() -- and as
//   per-thread lists merged at the end as the CPU backend does; for n_top of
//   1, 7, the stream's length and more than it.  The result must be the first
//   n_top of a plain std::sort of the whole stream by (score descending, rank
//   ascending), with the 0.0 / -1 fill behind a short list.
// It includes fs_pairscan.h only, links nothing of the library and needs no
// device.  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../fastselect_amd/csrc/fs_pairscan.h"

using namespace fs;

static long checks = 0;
static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    checks++;                                                                        \
    if (!(cond)) {                                                                   \
      if (failures < 20) std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      failures++;                                                                    \
    }                                                                                \
  } while (0)

static void check_keys() {
  const double inf = std::numeric_limits<double>::infinity();
  const double den = std::numeric_limits<double>::denorm_min();
  const double v[] = {-inf, -1e300, -2.5, -1.0, -1e-300, -den, -0.0, 0.0, den, 1e-300,
                      0.5, 1.0, 1.0000000000000002, 2.5, 1e300, inf};
  const int m = (int)(sizeof(v) / sizeof(v[0]));
  for (int a = 0; a < m; a++) {
    CHECK(pair_key(v[a]) != kPairNoKey);
    CHECK(pair_score(pair_key(v[a])) == v[a]);
    for (int b = 0; b < m; b++) {
      CHECK((v[a] < v[b]) == (pair_key(v[a]) < pair_key(v[b])));
      CHECK((v[a] == v[b]) == (pair_key(v[a]) == pair_key(v[b])));
    }
  }
  CHECK(pair_key(-0.0) == pair_key(0.0));
  CHECK(!std::signbit(pair_score(pair_key(-0.0))));
  // the order: score first, then the lower rank
  CHECK(pair_beats(pair_key(0.5), 9, pair_key(0.25), 1));
  CHECK(pair_beats(pair_key(0.5), 1, pair_key(0.5), 2));
  CHECK(!pair_beats(pair_key(0.5), 2, pair_key(0.5), 2));
  CHECK(pair_beats(pair_key(-0.0), 1, pair_key(0.0), 2));
  CHECK(!pair_beats(pair_key(0.0), 2, pair_key(-0.0), 1));
  CHECK(pair_beats(pair_key(-inf), 0, kPairNoKey, INT64_MAX));
}

static void check_ranks() {
  for (int64_t p = 2; p <= 70; p++) {
    int64_t r = 0;
    for (int64_t i = 0; i < p; i++)
      for (int64_t j = i + 1; j < p; j++, r++) {
        CHECK(pair_rank(p, i, j) == r);
        int64_t a = -1, b = -1;
        pair_unrank(p, r, a, b);
        CHECK(a == i && b == j);
      }
    CHECK(r == pair_count(p));
  }
  for (int64_t p : {(int64_t)65537, (int64_t)1000003, (int64_t)3000000000ll}) {
    const int64_t total = pair_count(p);
    const int64_t at[] = {0, 1, p - 2, p - 1, total / 2, total - 2, total - 1};
    for (int64_t r : at) {
      int64_t a = -1, b = -1;
      pair_unrank(p, r, a, b);
      CHECK(0 <= a && a < b && b < p && pair_rank(p, a, b) == r);
    }
  }
}

// a stream of (score, rank = position) and what a plain sort makes of it
struct Stream {
  std::vector<double> score;
  std::vector<PairCand> sorted;  // by (score descending, rank ascending)
  void finish() {
    sorted.clear();
    for (size_t r = 0; r < score.size(); r++) sorted.push_back(PairCand{pair_key(score[r]), (int64_t)r});
    std::sort(sorted.begin(), sorted.end(), [&](const PairCand& a, const PairCand& b) {
      const double sa = score[(size_t)a.rank], sb = score[(size_t)b.rank];
      return sa > sb || (sa == sb && a.rank < b.rank);
    });
  }
};

// the first n_top of the sort, with the fill, against what `top` holds; p is
// the column count whose C(p,2) covers the stream's ranks
static void check_list(const Stream& s, PairTopN& top, size_t n_top, int64_t p) {
  std::vector<double> sc(n_top, 9.0);
  std::vector<int64_t> ti(n_top, 9), tj(n_top, 9);
  top.sorted_into(p, sc.data(), ti.data(), tj.data());
  for (size_t t = 0; t < n_top; t++) {
    if (t < s.sorted.size()) {
      const int64_t r = s.sorted[t].rank;
      int64_t i, j;
      pair_unrank(p, r, i, j);
      CHECK(sc[t] == s.score[(size_t)r] && !std::signbit(sc[t] == 0.0 ? sc[t] : 1.0));
      CHECK(ti[t] == i && tj[t] == j);
    } else {
      CHECK(sc[t] == 0.0 && ti[t] == -1 && tj[t] == -1);
    }
  }
}

static void check_merge(const Stream& s, size_t n_top, size_t batch, int64_t p) {
  // the GPU backend's protocol: the threshold of a batch is the list's before it
  PairTopN top(n_top);
  for (size_t b0 = 0; b0 < s.score.size(); b0 += batch) {
    const PairCand thr = top.thr;
    const bool was_full = top.full;
    for (size_t r = b0; r < std::min(s.score.size(), b0 + batch); r++) {
      const uint64_t key = pair_key(s.score[r]);
      if (pair_beats(key, (int64_t)r, thr.key, thr.rank)) top.push(key, (int64_t)r);
      else CHECK(was_full);  // before the list is full every pair is a candidate
    }
    top.compact();
    CHECK(top.v.size() <= n_top || !top.full);
    CHECK(top.full == (std::min(s.score.size(), b0 + batch) >= n_top));
  }
  check_list(s, top, n_top, p);
  // the CPU backend's: contiguous runs, one list each, merged into the first
  for (size_t parts : {(size_t)1, (size_t)3, (size_t)16}) {
    std::vector<PairTopN> tops;
    for (size_t w = 0; w < parts; w++) tops.emplace_back(n_top);
    for (size_t w = 0; w < parts; w++)
      for (size_t r = s.score.size() * w / parts; r < s.score.size() * (w + 1) / parts; r++)
        tops[w].push(pair_key(s.score[r]), (int64_t)r);
    for (size_t w = 1; w < parts; w++) tops[0].merge(tops[w]);
    check_list(s, tops[0], n_top, p);
  }
}

int main() {
  check_keys();
  check_ranks();
  std::mt19937_64 rng(20240611);
  const int64_t p = 64;  // C(64, 2) = 2016 ranks
  const size_t len = 2016;
  for (int kind = 0; kind < 4; kind++) {
    Stream s;
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    for (size_t r = 0; r < len; r++) {
      double v;
      if (kind == 0) v = uni(rng);                                       // random keys
      else if (kind == 1) v = (double)(int)(rng() % 5) * 0.25 - 0.5;       // five values, zero among them
      else if (kind == 2) v = (rng() & 1) ? -0.0 : 0.0;                    // all equal to ==
      else v = (rng() % 3 == 0) ? uni(rng) : -0.125;                       // a mass below random ones
      s.score.push_back(v);
    }
    s.finish();
    for (size_t n_top : {(size_t)1, (size_t)7, (size_t)100, len, len + 5})
      for (size_t batch : {(size_t)1, (size_t)64, (size_t)256, (size_t)1000, len})
        check_merge(s, n_top, batch, p);
  }
  // lists shorter than n_top
  for (size_t shortlen : {(size_t)0, (size_t)1, (size_t)6}) {
    Stream s;
    for (size_t r = 0; r < shortlen; r++) s.score.push_back(r % 2 ? -0.5 : 0.0);
    s.finish();
    check_merge(s, 7, 4, p);
    check_merge(s, 65536, 256, p);
  }
  if (failures) {
    std::printf("pair_merge_selftest: FAILED %d of %ld checks\n", failures, checks);
    return 1;
  }
  std::printf("pair_merge_selftest: ok, %ld checks\n", checks);
  return 0;
}
