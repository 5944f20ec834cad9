// fs_mdr.hip -- the GPU backend of fs_mdr_scan (MDR.py:20-79 mdr_kernel, for
// every fold at once).
//
//   k_mdr_pack   X (bytes, uploaded once) -> genotype bit-planes in the
//                segment layout of fs_mdr.h: planes[(w * 3 + g) * p + j], u32
//                words, column index fastest.  Lanes that scan neighbouring
//                ranks differ in their last column only, so their plane loads
//                are consecutive words and the leading columns' loads are one
//                word for the whole wave.
//   k_mdr_scan   one lane per combination rank, unranked on the device from
//                its int64 rank.  Cell-major: for a cell of the first k-1
//                columns the lane walks the words segment by segment and keeps
//                popcount(AND) per (fold, class) for the last column's three
//                genotypes in registers; a fold's training counts are the
//                totals minus its own.  No 3^k table exists.  Up to kMdrG
//                folds per launch; more run in groups, each walking the other
//                folds' words for the totals.  A lane takes its ranks
//                in ascending order and keeps its best (BA bits, iteration);
//                the block reduces (max BA, min rank) per fold and merges it
//                into its slot of the partials, which the host reduces.  No
//                atomics: the result is deterministic.  A block owns a
//                contiguous run of ranks: a lane unranks once and then steps
//                its combination by the block size (mdr_advance).
#include "fs_gpu_internal.h"
#include "fs_mdr.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kMdrG = 16;          // folds held in registers per launch
constexpr int kMdrThreads = 256;
constexpr int kMdrMaxBlocks = 2048;
constexpr uint32_t kNoIter = 0xffffffffu;

// One thread per (word, column): 32 samples of one column -> three words.
__global__ __launch_bounds__(256) void k_mdr_pack(const uint8_t* __restrict__ x, int64_t p,
                                                  const int32_t* __restrict__ perm, int64_t words,
                                                  uint32_t* __restrict__ planes,
                                                  int* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = blockIdx.y;
  if (j >= p || w >= words) return;
  uint32_t b0 = 0, b1 = 0, b2 = 0;
  bool wrong = false;
  for (int b = 0; b < 32; b++) {
    const int32_t i = perm[w * 32 + b];
    if (i < 0) continue;
    const uint8_t g = x[(size_t)i * p + j];
    b0 |= (uint32_t)(g == 0) << b;
    b1 |= (uint32_t)(g == 1) << b;
    b2 |= (uint32_t)(g == 2) << b;
    wrong |= g > 2;
  }
  planes[((size_t)w * 3 + 0) * p + j] = b0;
  planes[((size_t)w * 3 + 1) * p + j] = b1;
  planes[((size_t)w * 3 + 2) * p + j] = b2;
  if (wrong) atomicOr(bad, 1);
}

struct MdrScanArgs {
  const uint32_t* planes;
  int64_t p;
  const int32_t* seg_off;   // 2F + 1 word offsets, segment c * F + f
  const int64_t* tc;        // F training cases
  const int64_t* tn;        // F training controls
  int F, f0, gn, sub;       // this launch scores folds [f0, f0 + gn)
  int64_t count, r0, r1;    // C(p,k) and this launch's rank range
  int64_t per_block;        // ranks per block, a multiple of the block size
  float* ba_out;            // NULL or F x count
  uint32_t* part_bits;      // kMdrMaxBlocks x F
  int64_t* part_rank;
};

// popcount(AND) over the words [w0, w1) for the last column's three genotypes
template <int K>
__device__ __forceinline__ void count3(const uint32_t* const* pre, const uint32_t* last,
                                       size_t p, int w0, int w1, uint32_t& a0, uint32_t& a1,
                                       uint32_t& a2) {
  for (int w = w0; w < w1; w++) {
    const size_t o = (size_t)w * 3 * p;
    uint32_t m = 0xffffffffu;
#pragma unroll
    for (int t = 0; t < K - 1; t++) m &= pre[t][o];
    a0 += __popc(m & last[o]);
    a1 += __popc(m & last[o + p]);
    a2 += __popc(m & last[o + 2 * p]);
  }
}

template <int K, int G>
__global__ __launch_bounds__(kMdrThreads) void k_mdr_scan(const MdrScanArgs a) {
  __shared__ uint32_t s_bits[kMdrThreads / 64];
  __shared__ int64_t s_rank[kMdrThreads / 64];
  const int tid = threadIdx.x;
  const int F = a.F, f0 = a.f0, gn = a.gn;
  const size_t p = (size_t)a.p;
  // the block owns a contiguous run of ranks and takes it 256 at a time
  const int64_t first = a.r0 + (int64_t)blockIdx.x * a.per_block + tid;
  const int64_t end = min(a.r1, a.r0 + ((int64_t)blockIdx.x + 1) * a.per_block);
  int cells = 1;
#pragma unroll
  for (int t = 1; t < K; t++) cells *= 3;

  uint32_t best_bits[G], best_it[G];
#pragma unroll
  for (int i = 0; i < G; i++) best_bits[i] = 0, best_it[i] = kNoIter;

  uint32_t it = 0;
  int32_t f[K];
  for (int64_t r = first; r < end; r += kMdrThreads, it++) {
    if (it == 0) mdr_unrank(a.p, K, r, f);
    else mdr_advance(a.p, K, f, kMdrThreads);
    uint32_t tp[G], tn[G];
#pragma unroll
    for (int i = 0; i < G; i++) tp[i] = tn[i] = 0;
    const uint32_t* last = a.planes + f[K - 1];
    for (int cell = 0; cell < cells; cell++) {
      const uint32_t* pre[K > 1 ? K - 1 : 1];
      {
        int c = cell;
#pragma unroll
        for (int t = K - 2; t >= 0; t--) {
          pre[t] = a.planes + (size_t)(c % 3) * p + f[t];
          c /= 3;
        }
      }
      uint32_t cc[3][G], ct[3][G], totc[3] = {0, 0, 0}, totn[3] = {0, 0, 0};
      if (gn < F) {  // the other folds' words count towards the totals only
        count3<K>(pre, last, p, a.seg_off[0], a.seg_off[f0], totc[0], totc[1], totc[2]);
        count3<K>(pre, last, p, a.seg_off[f0 + gn], a.seg_off[F], totc[0], totc[1], totc[2]);
        count3<K>(pre, last, p, a.seg_off[F], a.seg_off[F + f0], totn[0], totn[1], totn[2]);
        count3<K>(pre, last, p, a.seg_off[F + f0 + gn], a.seg_off[2 * F], totn[0], totn[1],
                  totn[2]);
      }
#pragma unroll
      for (int i = 0; i < G; i++) {
#pragma unroll
        for (int g = 0; g < 3; g++) cc[g][i] = ct[g][i] = 0;
        if (i < gn) {
          count3<K>(pre, last, p, a.seg_off[f0 + i], a.seg_off[f0 + i + 1], cc[0][i], cc[1][i],
                    cc[2][i]);
          count3<K>(pre, last, p, a.seg_off[F + f0 + i], a.seg_off[F + f0 + i + 1], ct[0][i],
                    ct[1][i], ct[2][i]);
#pragma unroll
          for (int g = 0; g < 3; g++) totc[g] += cc[g][i], totn[g] += ct[g][i];
        }
      }
#pragma unroll
      for (int i = 0; i < G; i++) {
        if (i < gn) {
          const uint64_t TC = (uint64_t)a.tc[f0 + i], TN = (uint64_t)a.tn[f0 + i];
#pragma unroll
          for (int g = 0; g < 3; g++) {
            const uint32_t cs = totc[g] - (a.sub ? cc[g][i] : 0);
            const uint32_t cn = totn[g] - (a.sub ? ct[g][i] : 0);
            const bool high = mdr_high_risk(cs, cn, TC, TN);
            tp[i] += high ? cs : 0;
            tn[i] += high ? 0 : cn;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < G; i++) {
      if (i < gn) {
        const float ba = mdr_ba(tp[i], tn[i], (uint64_t)a.tc[f0 + i], (uint64_t)a.tn[f0 + i]);
        if (a.ba_out) a.ba_out[(size_t)(f0 + i) * a.count + r] = ba;
        const uint32_t bits = __float_as_uint(ba);
        // ranks ascend with `it`, so a strict improvement keeps the smallest
        if (best_it[i] == kNoIter || bits > best_bits[i]) best_bits[i] = bits, best_it[i] = it;
      }
    }
  }

  // per fold: wave reduce, then the block's four waves, then the block's slot
#pragma unroll
  for (int i = 0; i < G; i++) {
    if (i < gn) {
      uint32_t bits = best_bits[i];
      int64_t rank = best_it[i] == kNoIter ? kMdrNoRank : first + (int64_t)best_it[i] * kMdrThreads;
      for (int d = 32; d > 0; d >>= 1) {
        const uint32_t ob = __shfl_xor(bits, d, 64);
        const int64_t orank = __shfl_xor((long long)rank, d, 64);
        if (mdr_better(ob, orank, bits, rank)) bits = ob, rank = orank;
      }
      if ((tid & 63) == 0) s_bits[tid >> 6] = bits, s_rank[tid >> 6] = rank;
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < kMdrThreads / 64; w++)
          if (mdr_better(s_bits[w], s_rank[w], bits, rank)) bits = s_bits[w], rank = s_rank[w];
        const size_t slot = (size_t)blockIdx.x * F + f0 + i;
        if (mdr_better(bits, rank, a.part_bits[slot], a.part_rank[slot]))
          a.part_bits[slot] = bits, a.part_rank[slot] = rank;
      }
      __syncthreads();
    }
  }
}

template <int K>
void launch_scan(const MdrScanArgs& a, int blocks, hipStream_t s) {
  if (a.F == 1)
    k_mdr_scan<K, 1><<<blocks, kMdrThreads, 0, s>>>(a);
  else
    k_mdr_scan<K, kMdrG><<<blocks, kMdrThreads, 0, s>>>(a);
}

}  // namespace

int mdr_scan(int device, const uint8_t* x, int64_t n, int64_t p, const uint8_t* is_case, int k,
             const int32_t* fold, int n_folds, int64_t count, float* best_ba, int64_t* best_rank,
             float* ba_out) {
  if (device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  MdrLayout L;
  if (int rc = mdr_layout(n, is_case, fold, n_folds, 32, L)) return rc;
  const int F = L.F;
  const int64_t W = L.words;
  const size_t nslots = (size_t)kMdrMaxBlocks * F;
  std::vector<uint32_t> h_bits(nslots, 0);
  std::vector<int64_t> h_rank(nslots, kMdrNoRank);

  uint8_t* dx = nullptr;
  int32_t *dperm = nullptr, *dseg = nullptr;
  int64_t *dtc = nullptr, *dtn = nullptr, *dprank = nullptr;
  uint32_t *dplanes = nullptr, *dpbits = nullptr;
  float* dba = nullptr;
  int* dbad = nullptr;
  hipStream_t s = nullptr;
  int rc = FS_OK;
  auto fail = [&](const char* what, hipError_t e) {
    set_error(std::string("fs_mdr_scan: ") + what + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
    rc = (e == hipErrorOutOfMemory) ? FS_EOOM : FS_EHIP;
  };
  auto up = [&](void* dst, const void* src, size_t bytes, const char* what) {
    hipError_t e;
    if (rc == FS_OK && (e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
      fail(what, e);
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) fail("hipSetDevice", e);
  if (rc == FS_OK && (e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess)
    fail("hipStreamCreate", e);
  const size_t plane_words = (size_t)W * 3 * (size_t)p;
  DevArena mem(device);  // freed on return, after the stream is synchronised
  if (rc == FS_OK) rc = mem.alloc(&dx, (size_t)n * p);
  if (rc == FS_OK) rc = mem.alloc(&dperm, L.perm.size());
  if (rc == FS_OK) rc = mem.alloc(&dseg, L.seg_off.size());
  if (rc == FS_OK) rc = mem.alloc(&dtc, (size_t)F);
  if (rc == FS_OK) rc = mem.alloc(&dtn, (size_t)F);
  if (rc == FS_OK) rc = mem.alloc(&dplanes, plane_words);
  if (rc == FS_OK) rc = mem.alloc(&dpbits, nslots);
  if (rc == FS_OK) rc = mem.alloc(&dprank, nslots);
  if (rc == FS_OK) rc = mem.alloc(&dbad, 1);
  if (rc == FS_OK && ba_out) rc = mem.alloc(&dba, (size_t)F * count);
  up(dx, x, (size_t)n * p, "upload of X");
  up(dperm, L.perm.data(), L.perm.size() * 4, "upload of the sample order");
  up(dseg, L.seg_off.data(), L.seg_off.size() * 4, "upload of the segments");
  up(dtc, L.tc.data(), (size_t)F * 8, "upload of the totals");
  up(dtn, L.tn.data(), (size_t)F * 8, "upload of the totals");
  up(dpbits, h_bits.data(), nslots * 4, "upload of the partials");
  up(dprank, h_rank.data(), nslots * 8, "upload of the partials");
  if (rc == FS_OK && (e = hipMemsetAsync(dbad, 0, 4, s)) != hipSuccess) fail("hipMemset", e);

  if (rc == FS_OK) {
    // grid.y is limited to 65535: pack the words in slabs
    const unsigned gx = (unsigned)((p + 255) / 256);
    for (int64_t w0 = 0; w0 < W && rc == FS_OK; w0 += 65535) {
      const int64_t wn = std::min<int64_t>(65535, W - w0);
      k_mdr_pack<<<dim3(gx, (unsigned)wn), 256, 0, s>>>(dx, p, dperm + w0 * 32, wn,
                                                        dplanes + (size_t)w0 * 3 * p, dbad);
      if ((e = hipGetLastError()) != hipSuccess) fail("pack kernel", e);
    }
  }
  int bad = 0;
  if (rc == FS_OK && ((e = hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
                      (e = hipStreamSynchronize(s)) != hipSuccess))
    fail("pack", e);
  if (rc == FS_OK && bad) {
    set_error("fs_mdr_scan: genotypes must be coded 0/1/2");
    rc = FS_EINVAL;
  }

  if (rc == FS_OK) {
    // launches of about 2e11 lane operations each (a few milliseconds at the
    // VALU peak), so that no launch holds the device for long
    int cells = 1;
    for (int t = 1; t < k; t++) cells *= 3;
    const int groups = (F + kMdrG - 1) / kMdrG;
    const double ops = (double)cells * (double)W * (k + 5) * (groups > 1 ? 2.0 : 1.0);
    int64_t chunk = (int64_t)std::max(65536.0, std::min(2e11 / ops, 4e18));
    MdrScanArgs a;
    a.planes = dplanes, a.p = p, a.seg_off = dseg, a.tc = dtc, a.tn = dtn;
    a.F = F, a.sub = L.sub, a.count = count, a.ba_out = dba;
    a.part_bits = dpbits, a.part_rank = dprank;
    for (int64_t r0 = 0; r0 < count && rc == FS_OK; r0 += chunk) {
      a.r0 = r0, a.r1 = std::min(count, r0 + chunk);
      const int blocks = (int)std::min<int64_t>(
          kMdrMaxBlocks, (a.r1 - a.r0 + kMdrThreads - 1) / kMdrThreads);
      const int64_t iters = (a.r1 - a.r0 + (int64_t)blocks * kMdrThreads - 1) /
                            ((int64_t)blocks * kMdrThreads);
      a.per_block = iters * kMdrThreads;
      for (int f0 = 0; f0 < F && rc == FS_OK; f0 += kMdrG) {
        a.f0 = f0, a.gn = std::min(kMdrG, F - f0);
        switch (k) {
          case 1: launch_scan<1>(a, blocks, s); break;
          case 2: launch_scan<2>(a, blocks, s); break;
          case 3: launch_scan<3>(a, blocks, s); break;
          case 4: launch_scan<4>(a, blocks, s); break;
          case 5: launch_scan<5>(a, blocks, s); break;
          default: launch_scan<6>(a, blocks, s); break;
        }
        if ((e = hipGetLastError()) != hipSuccess) fail("scan kernel", e);
      }
    }
  }
  if (rc == FS_OK &&
      ((e = hipMemcpyAsync(h_bits.data(), dpbits, nslots * 4, hipMemcpyDeviceToHost, s)) !=
           hipSuccess ||
       (e = hipMemcpyAsync(h_rank.data(), dprank, nslots * 8, hipMemcpyDeviceToHost, s)) !=
           hipSuccess))
    fail("download of the partials", e);
  if (rc == FS_OK && ba_out &&
      (e = hipMemcpyAsync(ba_out, dba, (size_t)F * count * 4, hipMemcpyDeviceToHost, s)) !=
          hipSuccess)
    fail("download of the balanced accuracies", e);
  if (rc == FS_OK && (e = hipStreamSynchronize(s)) != hipSuccess) fail("scan", e);
  if (s) (void)hipStreamSynchronize(s);
  if (rc == FS_OK)
    for (int i = 0; i < F; i++) {
      uint32_t bits = 0;
      int64_t rank = kMdrNoRank;
      for (int b = 0; b < kMdrMaxBlocks; b++) {
        const size_t slot = (size_t)b * F + i;
        if (mdr_better(h_bits[slot], h_rank[slot], bits, rank))
          bits = h_bits[slot], rank = h_rank[slot];
      }
      memcpy(&best_ba[i], &bits, 4);
      best_rank[i] = rank;
    }
  if (s) (void)hipStreamDestroy(s);
  return rc;
}

}  // namespace gpu
}  // namespace fs
