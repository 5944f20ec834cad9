// fs_mi.hip -- the GPU backend of fs_mi_matrices: the p x p matrix of pairwise
// discrete mutual information and the relevance vector in one tiled scan
// (replaces _mi_pair_gpu_kernel and the _batch_mi_cpu call that the
// reference's GPU path falls back to, mutual_information.py:70-115, 184-193).
//
//   k_mi_pack   codes (bytes, uploaded once) and y (as column p) -> state
//               bit-planes, word-major: planes[(w * P1p + c) * SP + s], u32
//               words over the samples, SP = n_states rounded up to 4, the
//               columns padded to whole tiles.  Padding bits, padding states
//               and padding columns are zero, so no mask is ever needed.  A
//               tile's planes of one word are SP * T consecutive words: the
//               scan stages them with 16-byte loads and the pack writes them
//               coalesced.  Also each column's state count (max code + 1, the
//               reference's k1) and a flag for a code >= n_states.
//   k_mi_scan   one workgroup per tile (column block I) x (column block J),
//               I <= J, T columns each.  Per chunk of kMiWC words it stages
//               both blocks' planes in LDS, [word][column][state], and every
//               lane accumulates popcount(plane_i[a] & plane_j[b]) for ONE
//               4 x 4 block of ONE pair's table in 16 registers, both operands
//               from LDS with one 16-byte read each.  A pair takes NB^2 lanes
//               (NB = SP / 4 blocks a side), so T = 16 / NB and T * SP <= 64:
//               16 x 16 pairs at up to 4 states, 2 x 2 pairs at 32.  The
//               epilogue runs in the same kernel on the same lanes: pxy into
//               LDS (over the dead staging area), the marginals in index
//               order, every cell's term on the lane that counted it, and the
//               pair's first lane adds the terms row-major (fs_mi.h) and
//               writes redundancy[i][j], [j][i] or relevance[i].  No table
//               reaches HBM unless counts_out is asked for; no atomics touch
//               a result.
#include "fs_gpu_internal.h"
#include "fs_mi.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kMiThreads = 256;
constexpr int kMiWC = 64;          // words (2048 samples) staged per chunk
constexpr int kMiRow = 64;         // most words of one staged word row: T * SP
constexpr int kMiMarg = 1024;      // most marginals of a tile: T * T * SP

thread_local double g_mi_ms[4] = {-1.0, -1.0, -1.0, -1.0};

// One thread per (column, word): 32 samples of one column -> SP words.
__global__ __launch_bounds__(256) void k_mi_pack(const uint8_t* __restrict__ x,
                                                 const uint8_t* __restrict__ y, int64_t n,
                                                 int64_t p, int64_t P1p, int S, int SP, int64_t w0,
                                                 uint32_t* __restrict__ planes,
                                                 int32_t* __restrict__ kcol,
                                                 int* __restrict__ bad) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t w = w0 + blockIdx.y;
  if (c >= P1p) return;
  uint32_t code[32];
  uint32_t mx = 0;
#pragma unroll
  for (int b = 0; b < 32; b++) {
    const int64_t i = w * 32 + b;
    uint32_t g = 0xffffffffu;  // padding: matches no state
    if (i < n && c <= p) {
      g = c < p ? x[(size_t)i * p + c] : y[i];
      mx = g > mx ? g : mx;
    }
    code[b] = g;
  }
  uint32_t* out = planes + ((size_t)w * P1p + c) * SP;
  for (int s = 0; s < SP; s++) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 32; b++) word |= (uint32_t)(code[b] == (uint32_t)s) << b;
    out[s] = word;
  }
  if (c <= p) {
    if (mx >= (uint32_t)S) atomicOr(bad, 1);
    atomicMax(&kcol[c], (int32_t)mx + 1);
  }
}

struct MiScanArgs {
  const uint32_t* planes;
  const int32_t* kcol;      // P1 state counts
  int64_t n, p, P1p, W;
  int S, SP, NB, T;
  int64_t nbt;              // column blocks: P1p / T
  int64_t t0;               // first tile of this launch
  int only_y;               // tiles (t, nbt - 1) and the pairs with y alone
  int unit;
  double* red;              // p x p (NULL with only_y)
  double* rel;              // p
  int32_t* counts;          // NULL or p x p x S x S
};

// tile t of the upper triangle (row-major, diagonal included) -> (bi, bj)
__device__ __forceinline__ void mi_tile(int64_t nb, int64_t t, int64_t& bi, int64_t& bj) {
  const double m = 2.0 * (double)nb + 1.0;
  int64_t r = (int64_t)((m - sqrt(m * m - 8.0 * (double)t)) * 0.5);
  r = r < 0 ? 0 : (r > nb - 1 ? nb - 1 : r);
  while (r > 0 && tile_linear(nb, r, r) > t) r--;
  while (r + 1 < nb && tile_linear(nb, r + 1, r + 1) <= t) r++;
  bi = r;
  bj = r + (t - tile_linear(nb, r, r));
}

__global__ __launch_bounds__(kMiThreads) void k_mi_scan(const MiScanArgs a) {
  // staging: [side][word][T * SP]; after the scan: the tile's pxy, then terms
  __shared__ __align__(16) uint32_t s_raw[2 * kMiWC * kMiRow];
  __shared__ double s_p1[kMiMarg];
  __shared__ double s_p2[kMiMarg];
  const int tid = threadIdx.x;
  const int SP = a.SP, NB = a.NB, T = a.T;
  const int NP = T * SP;       // words of one staged word row
  const int nv = NP / 4;       // ... in 16-byte vectors
  const int L = NB * NB;       // lanes per pair
  int64_t bi, bj;
  if (a.only_y) {
    bi = a.t0 + blockIdx.x;
    bj = a.nbt - 1;
  } else {
    mi_tile(a.nbt, a.t0 + blockIdx.x, bi, bj);
  }
  const int q = tid / L, blk = tid - q * L;
  const int ab = blk / NB, bb = blk - ab * NB;
  const int ii = q / T, jj = q - ii * T;
  const bool lane_on = q < T * T;
  const int64_t i = bi * T + ii, j = bj * T + jj;
  const bool pair_on = lane_on && i < j && j <= a.p && (!a.only_y || j == a.p);

  uint32_t c[16];
#pragma unroll
  for (int k = 0; k < 16; k++) c[k] = 0;

  const size_t row = (size_t)a.P1p * SP;  // words of one word row in HBM
  const uint32_t* gi = a.planes + (size_t)bi * NP;
  const uint32_t* gj = a.planes + (size_t)bj * NP;
  uint4* si = reinterpret_cast<uint4*>(s_raw);
  uint4* sj = reinterpret_cast<uint4*>(s_raw + kMiWC * kMiRow);
  const int oi = (ii * SP + 4 * ab) / 4, oj = (jj * SP + 4 * bb) / 4;
  for (int64_t w0 = 0; w0 < a.W; w0 += kMiWC) {
    const int wn = a.W - w0 < kMiWC ? (int)(a.W - w0) : kMiWC;
    for (int v = tid; v < wn * nv; v += kMiThreads) {
      const int w = v / nv, xq = v - w * nv;
      const size_t g = (size_t)(w0 + w) * row + 4 * (size_t)xq;
      si[v] = *reinterpret_cast<const uint4*>(gi + g);
      sj[v] = *reinterpret_cast<const uint4*>(gj + g);
    }
    __syncthreads();
    if (pair_on) {
      for (int w = 0; w < wn; w++) {
        const uint4 A = si[w * nv + oi], B = sj[w * nv + oj];
        c[0] += __builtin_popcount(A.x & B.x);
        c[1] += __builtin_popcount(A.x & B.y);
        c[2] += __builtin_popcount(A.x & B.z);
        c[3] += __builtin_popcount(A.x & B.w);
        c[4] += __builtin_popcount(A.y & B.x);
        c[5] += __builtin_popcount(A.y & B.y);
        c[6] += __builtin_popcount(A.y & B.z);
        c[7] += __builtin_popcount(A.y & B.w);
        c[8] += __builtin_popcount(A.z & B.x);
        c[9] += __builtin_popcount(A.z & B.y);
        c[10] += __builtin_popcount(A.z & B.z);
        c[11] += __builtin_popcount(A.z & B.w);
        c[12] += __builtin_popcount(A.w & B.x);
        c[13] += __builtin_popcount(A.w & B.y);
        c[14] += __builtin_popcount(A.w & B.z);
        c[15] += __builtin_popcount(A.w & B.w);
      }
    }
    __syncthreads();
  }

  if (a.counts && pair_on && j < a.p) {
    int32_t* out = a.counts + ((size_t)i * a.p + j) * a.S * a.S;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (4 * ab + r < a.S && 4 * bb + k < a.S)
          out[(size_t)(4 * ab + r) * a.S + 4 * bb + k] = (int32_t)c[r * 4 + k];
  }

  // epilogue (fs_mi.h): pxy, marginals in index order, terms, row-major sum
  double* s_px = reinterpret_cast<double*>(s_raw);  // [pair][SP][SP], <= 4096 doubles
  const double dn = (double)a.n;
  const int tb = q * SP * SP + 4 * ab * SP + 4 * bb;
  double px[16];
#pragma unroll
  for (int k = 0; k < 16; k++) px[k] = mi_pxy((int32_t)c[k], dn);
  if (lane_on) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) s_px[tb + r * SP + k] = px[r * 4 + k];
  }
  __syncthreads();
  for (int it = tid; it < T * T * SP; it += kMiThreads) {
    const int q2 = it / SP, s = it - q2 * SP;
    const double* t = s_px + q2 * SP * SP;
    double r1 = 0.0, r2 = 0.0;
    for (int b = 0; b < SP; b++) r1 += t[s * SP + b];
    for (int b = 0; b < SP; b++) r2 += t[b * SP + s];
    s_p1[it] = r1;
    s_p2[it] = r2;
  }
  __syncthreads();
  if (pair_on) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        s_px[tb + r * SP + k] =
            mi_term(px[r * 4 + k], s_p1[q * SP + 4 * ab + r], s_p2[q * SP + 4 * bb + k]);
  }
  __syncthreads();
  if (pair_on && blk == 0) {
    const int k1 = a.kcol[i], k2 = a.kcol[j];
    const double* t = s_px + q * SP * SP;
    double mi = 0.0;
    for (int r = 0; r < k1; r++)
      for (int k = 0; k < k2; k++) mi += t[r * SP + k];
    int used1 = 0, used2 = 0;
    for (int r = 0; r < k1; r++) used1 += s_p1[q * SP + r] > 0.0;
    for (int k = 0; k < k2; k++) used2 += s_p2[q * SP + k] > 0.0;
    mi = mi_constant(used1, used2) ? 0.0 : mi_finish(mi, a.unit);
    if (j == a.p) {
      a.rel[i] = mi;
    } else if (a.red) {
      a.red[(size_t)i * a.p + j] = mi;
      a.red[(size_t)j * a.p + i] = mi;
    }
  }
}

}  // namespace

hipError_t mi_pack(const uint8_t* x, const uint8_t* y, int64_t n, int64_t p, int64_t P1p, int S,
                   int SP, uint32_t* planes, int32_t* kcol, int* bad, hipStream_t s) {
  // grid.y is limited to 65535: pack the words in slabs
  const int64_t W = (n + 31) / 32;
  const unsigned gx = (unsigned)((P1p + 255) / 256);
  for (int64_t w0 = 0; w0 < W; w0 += 65535) {
    const int64_t wn = std::min<int64_t>(65535, W - w0);
    k_mi_pack<<<dim3(gx, (unsigned)wn), 256, 0, s>>>(x, y, n, p, P1p, S, SP, w0, planes, kcol,
                                                     bad);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

void mi_last_timing(double* ms4) {
  for (int k = 0; k < 4; k++) ms4[k] = g_mi_ms[k];
}

int mi_matrices(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, double* relevance, double* redundancy,
                int32_t* counts_out) {
  if (device_count() <= 0) {
    set_error("backend='gpu' requested but no HIP device is visible");
    return FS_ENODEV;
  }
  for (double& v : g_mi_ms) v = -1.0;
  const int S = n_states;
  const int NB = (S + 3) / 4, SP = NB * 4, T = 16 / NB;
  const int64_t P1 = p + 1;
  const int64_t nbt = (P1 + T - 1) / T, P1p = nbt * T;
  const int64_t W = (n + 31) / 32;
  // sizes in floating point first: a request beyond any device is an
  // out-of-memory answer, not an overflowed size
  const double kMaxBytes = 1e15;
  const double red_bytes = redundancy ? (double)p * (double)p * 8.0 : 0.0;
  const double cnt_bytes = counts_out ? (double)p * (double)p * (double)S * S * 4.0 : 0.0;
  const double pl_bytes = (double)W * (double)P1p * SP * 4.0;
  if (red_bytes > kMaxBytes || cnt_bytes > kMaxBytes || pl_bytes > kMaxBytes ||
      (double)n * (double)p > kMaxBytes) {
    set_error("fs_mi_matrices: the matrices do not fit the device memory");
    return FS_EOOM;
  }
  const size_t nred = redundancy ? (size_t)p * p : 0;
  const size_t ncnt = counts_out ? (size_t)p * p * S * S : 0;
  const size_t plane_words = (size_t)W * P1p * SP;

  uint8_t *dx = nullptr, *dy = nullptr;
  uint32_t* dplanes = nullptr;
  int32_t *dkcol = nullptr, *dcnt = nullptr;
  double *dred = nullptr, *drel = nullptr;
  int* dbad = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = FS_OK;
  auto fail = [&](const char* what, hipError_t e) {
    set_error(std::string("fs_mi_matrices: ") + what + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
    rc = (e == hipErrorOutOfMemory) ? FS_EOOM : FS_EHIP;
  };
  auto mark = [&](int k) {
    hipError_t e;
    if (rc == FS_OK && (e = hipEventRecord(ev[k], s)) != hipSuccess) fail("hipEventRecord", e);
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) fail("hipSetDevice", e);
  if (rc == FS_OK && (e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess)
    fail("hipStreamCreate", e);
  for (int k = 0; k < 5 && rc == FS_OK; k++)
    if ((e = hipEventCreate(&ev[k])) != hipSuccess) fail("hipEventCreate", e);
  DevArena mem(device);  // freed on return, after the stream is synchronised
  if (rc == FS_OK) rc = mem.alloc(&dx, (size_t)n * p);
  if (rc == FS_OK) rc = mem.alloc(&dy, (size_t)n);
  if (rc == FS_OK) rc = mem.alloc(&dplanes, plane_words);
  if (rc == FS_OK) rc = mem.alloc(&dkcol, (size_t)P1);
  if (rc == FS_OK) rc = mem.alloc(&drel, (size_t)p);
  if (rc == FS_OK) rc = mem.alloc(&dbad, 1);
  if (rc == FS_OK && nred) rc = mem.alloc(&dred, nred);
  if (rc == FS_OK && ncnt) rc = mem.alloc(&dcnt, ncnt);

  mark(0);
  if (rc == FS_OK && ((e = hipMemcpyAsync(dx, codes, (size_t)n * p, hipMemcpyHostToDevice, s)) !=
                          hipSuccess ||
                      (e = hipMemcpyAsync(dy, ycodes, (size_t)n, hipMemcpyHostToDevice, s)) !=
                          hipSuccess))
    fail("upload of the codes", e);
  if (rc == FS_OK && ((e = hipMemsetAsync(dbad, 0, 4, s)) != hipSuccess ||
                      (e = hipMemsetAsync(dkcol, 0, (size_t)P1 * 4, s)) != hipSuccess))
    fail("hipMemset", e);
  // the diagonal, and every cell of counts_out that no pair writes, stay zero
  if (rc == FS_OK && nred && (e = hipMemsetAsync(dred, 0, nred * 8, s)) != hipSuccess)
    fail("hipMemset", e);
  if (rc == FS_OK && ncnt && (e = hipMemsetAsync(dcnt, 0, ncnt * 4, s)) != hipSuccess)
    fail("hipMemset", e);
  mark(1);

  if (rc == FS_OK && (e = mi_pack(dx, dy, n, p, P1p, S, SP, dplanes, dkcol, dbad, s)) != hipSuccess)
    fail("pack kernel", e);
  mark(2);
  int bad = 0;
  if (rc == FS_OK && ((e = hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s)) != hipSuccess ||
                      (e = hipStreamSynchronize(s)) != hipSuccess))
    fail("pack", e);
  if (rc == FS_OK && bad) {
    set_error("fs_mi_matrices: a code is >= n_states");
    rc = FS_EINVAL;
  }

  if (rc == FS_OK) {
    // launches of about 2e11 lane operations each (a few milliseconds at the
    // VALU peak), so that no launch holds the device for long: per tile and
    // word 256 lanes run 16 ANDs and 16 popcount-accumulates
    MiScanArgs a;
    a.planes = dplanes, a.kcol = dkcol, a.n = n, a.p = p, a.P1p = P1p, a.W = W;
    a.S = S, a.SP = SP, a.NB = NB, a.T = T, a.nbt = nbt, a.unit = unit;
    a.only_y = nred == 0 && ncnt == 0;
    a.red = dred, a.rel = drel, a.counts = dcnt;
    const int64_t tiles = a.only_y ? nbt : nbt * (nbt + 1) / 2;
    const double ops = 256.0 * 32.0 * (double)W;
    int64_t per = (int64_t)std::max(1024.0, std::min(2e11 / ops, 1e9));
    if (test_hooks().mi_tiles > 0) per = test_hooks().mi_tiles;
    for (int64_t t0 = 0; t0 < tiles && rc == FS_OK; t0 += per) {
      a.t0 = t0;
      const unsigned blocks = (unsigned)std::min<int64_t>(per, tiles - t0);
      k_mi_scan<<<blocks, kMiThreads, 0, s>>>(a);
      if ((e = hipGetLastError()) != hipSuccess) fail("scan kernel", e);
    }
  }
  mark(3);
  if (rc == FS_OK &&
      (e = hipMemcpyAsync(relevance, drel, (size_t)p * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    fail("download of the relevance", e);
  if (rc == FS_OK && nred &&
      (e = hipMemcpyAsync(redundancy, dred, nred * 8, hipMemcpyDeviceToHost, s)) != hipSuccess)
    fail("download of the redundancy matrix", e);
  if (rc == FS_OK && ncnt &&
      (e = hipMemcpyAsync(counts_out, dcnt, ncnt * 4, hipMemcpyDeviceToHost, s)) != hipSuccess)
    fail("download of the counts", e);
  mark(4);
  if (rc == FS_OK && (e = hipStreamSynchronize(s)) != hipSuccess) fail("scan", e);
  if (s) (void)hipStreamSynchronize(s);
  if (rc == FS_OK)
    for (int k = 0; k < 4; k++) {
      float ms = -1.0f;
      if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_mi_ms[k] = ms;
    }
  (void)hipGetLastError();
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  if (s) (void)hipStreamDestroy(s);
  return rc;
}

}  // namespace gpu
}  // namespace fs
