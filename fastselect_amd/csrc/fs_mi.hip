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
//               I <= J, T columns each.  Per chunk of kPtWC words it stages
//               both blocks' planes in LDS, [word][column][state], and every
//               lane accumulates popcount(plane_i[a] & plane_j[b]) for ONE
//               4 x 4 block of ONE pair's table in 16 registers (pt_count,
//               fs_pairtab.h), both operands from LDS with one 16-byte read
//               each.  A pair takes NB^2 lanes (NB = SP / 4 blocks a side), so
//               T = 16 / NB and T * SP <= 64: 16 x 16 pairs at up to 4 states,
//               2 x 2 pairs at 32.  The epilogue runs in the same kernel on
//               the same lanes: pxy into LDS (over the dead staging area),
//               the marginals in index order, every cell's term on the lane
//               that counted it, and the pair's first lane adds the terms
//               row-major (fs_mi.h) and writes redundancy[i][j], [j][i] or
//               relevance[i].  These are the steps of pt_epilogue
//               (fs_pairtab.h, which k_cfs_row and k_mi_row run) in a copy of
//               this kernel's own, kept on a measurement: the note in the
//               kernel.  No table reaches HBM unless counts_out is asked for;
//               no atomics touch a result.
// The host side of "codes to packed planes" (MiPlanes, fs_mi.h) is here too.
#include "fs_gpu_internal.h"
#include "fs_mi.h"
#include "fs_pairtab.h"

namespace fs {
namespace gpu {

namespace {

constexpr int kMiRow = 64;         // most words of one staged word row: T * SP

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

__global__ __launch_bounds__(kPtThreads) void k_mi_scan(const MiScanArgs a) {
  // staging: [side][word][T * SP]; after the scan: the tile's pxy, then terms
  __shared__ __align__(16) uint32_t s_raw[2 * kPtWC * kMiRow];
  __shared__ double s_p1[kPtMarg];
  __shared__ double s_p2[kPtMarg];
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
  PtLane g;
  g.q = tid / L;
  const int blk = tid - g.q * L;
  g.ab = blk / NB, g.bb = blk - g.ab * NB;
  const int ii = g.q / T, jj = g.q - ii * T;
  g.lane_on = g.q < T * T;
  const int64_t i = bi * T + ii, j = bj * T + jj;
  g.pair_on = g.lane_on && i < j && j <= a.p && (!a.only_y || j == a.p);

  uint32_t c[16];
#pragma unroll
  for (int k = 0; k < 16; k++) c[k] = 0;

  const size_t row = (size_t)a.P1p * SP;  // words of one word row in HBM
  const uint32_t* gi = a.planes + (size_t)bi * NP;
  const uint32_t* gj = a.planes + (size_t)bj * NP;
  uint4* si = reinterpret_cast<uint4*>(s_raw);
  uint4* sj = reinterpret_cast<uint4*>(s_raw + kPtWC * kMiRow);
  const int oi = (ii * SP + 4 * g.ab) / 4, oj = (jj * SP + 4 * g.bb) / 4;
  for (int64_t w0 = 0; w0 < a.W; w0 += kPtWC) {
    const int wn = a.W - w0 < kPtWC ? (int)(a.W - w0) : kPtWC;
    for (int v = tid; v < wn * nv; v += kPtThreads) {
      const int w = v / nv, xq = v - w * nv;
      const size_t gw = (size_t)(w0 + w) * row + 4 * (size_t)xq;
      si[v] = *reinterpret_cast<const uint4*>(gi + gw);
      sj[v] = *reinterpret_cast<const uint4*>(gj + gw);
    }
    __syncthreads();
    if (g.pair_on)
      for (int w = 0; w < wn; w++) pt_count(si[w * nv + oi], sj[w * nv + oj], c);
    __syncthreads();
  }

  if (a.counts && g.pair_on && j < a.p) {
    int32_t* out = a.counts + ((size_t)i * a.p + j) * a.S * a.S;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (4 * g.ab + r < a.S && 4 * g.bb + k < a.S)
          out[(size_t)(4 * g.ab + r) * a.S + 4 * g.bb + k] = (int32_t)c[r * 4 + k];
  }

  // The epilogue: pt_epilogue's steps (fs_pairtab.h) without the transposition
  // (i < j always), in this kernel's own copy.  Instantiating the shared
  // function here gave the same instructions in another schedule and measured
  // slower against the parent build on 2000 x 5000 x 3: the kernel 1907-1925 us
  // against 1899-1900 us, the scan phase 1.96-1.98 ms against 1.93-1.97 ms, in
  // four sessions; this copy measured 1888-1905 us and 1.93-1.95 ms
  // (profiles/pairtab/README.md).  Whoever changes one of the two changes the
  // other: tests/test_gpu_mrmr_selected.py asserts that k_mi_row's values equal
  // this kernel's bit for bit.  The tile's pxy and terms go over the dead
  // staging area.
  double* s_px = reinterpret_cast<double*>(s_raw);  // [pair][SP][SP], <= 4096 doubles
  const double dn = (double)a.n;
  const int q = g.q;
  const int tb = q * SP * SP + 4 * g.ab * SP + 4 * g.bb;
  double px[16];
#pragma unroll
  for (int k = 0; k < 16; k++) px[k] = mi_pxy((int32_t)c[k], dn);
  if (g.lane_on) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) s_px[tb + r * SP + k] = px[r * 4 + k];
  }
  __syncthreads();
  for (int it = tid; it < T * T * SP; it += kPtThreads) {
    const int q2 = it / SP, s = it - q2 * SP;
    const double* t = s_px + q2 * SP * SP;
    double r1 = 0.0, r2 = 0.0;
    for (int b = 0; b < SP; b++) r1 += t[s * SP + b];
    for (int b = 0; b < SP; b++) r2 += t[b * SP + s];
    s_p1[it] = r1;
    s_p2[it] = r2;
  }
  __syncthreads();
  if (g.pair_on) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int k = 0; k < 4; k++)
        s_px[tb + r * SP + k] =
            mi_term(px[r * 4 + k], s_p1[q * SP + 4 * g.ab + r], s_p2[q * SP + 4 * g.bb + k]);
  }
  __syncthreads();
  if (g.pair_on && blk == 0) {
    // the state counts bounded by SP, as in pt_epilogue
    const int k1 = a.kcol[i] < SP ? a.kcol[i] : SP, k2 = a.kcol[j] < SP ? a.kcol[j] : SP;
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

int MiPlanes::shape(const char* who_, int64_t n_, int64_t p_, int n_states, int pad) {
  who = who_, n = n_, p = p_, S = n_states;
  NB = (S + 3) / 4, SP = NB * 4;
  P1 = p + 1, P1p = (P1 + pad - 1) / pad * pad;
  W = (n + 31) / 32;
  // sizes in floating point first: a request beyond any device is an
  // out-of-memory answer, not an overflowed size
  if ((double)W * (double)P1p * SP * 4.0 > kMiMaxBytes || (double)n * (double)p > kMiMaxBytes) {
    set_error(std::string(who) + ": the bit-planes do not fit the device memory");
    return FS_EOOM;
  }
  return FS_OK;
}

int MiPlanes::alloc(DevArena& mem, DevArena& up) {
  FS_TRY(up.alloc(&dx, (size_t)n * p));
  FS_TRY(up.alloc(&dy, (size_t)n));
  FS_TRY(mem.alloc(&planes, (size_t)W * P1p * SP));
  FS_TRY(mem.alloc(&kcol, (size_t)P1));
  return mem.alloc(&dbad, 1);
}

int MiPlanes::upload(const uint8_t* codes, const uint8_t* ycodes, hipStream_t s) {
  FS_HIP(hipMemcpyAsync(dx, codes, (size_t)n * p, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemcpyAsync(dy, ycodes, (size_t)n, hipMemcpyHostToDevice, s));
  FS_HIP(hipMemsetAsync(dbad, 0, 4, s));
  FS_HIP(hipMemsetAsync(kcol, 0, (size_t)P1 * 4, s));  // k_mi_pack takes maxima
  return FS_OK;
}

int MiPlanes::pack(hipStream_t s) {
  // grid.y is limited to 65535: pack the words in slabs
  const unsigned gx = (unsigned)((P1p + 255) / 256);
  for (int64_t w0 = 0; w0 < W; w0 += 65535) {
    const int64_t wn = std::min<int64_t>(65535, W - w0);
    k_mi_pack<<<dim3(gx, (unsigned)wn), 256, 0, s>>>(dx, dy, n, p, P1p, S, SP, w0, planes, kcol,
                                                     dbad);
    FS_TRY(launch_check("k_mi_pack"));
  }
  return FS_OK;
}

int MiPlanes::fetch_bad(hipStream_t s) {
  FS_HIP(hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s));
  return FS_OK;
}

int MiPlanes::check() const {
  if (!bad) return FS_OK;
  set_error(std::string(who) + ": a code is >= n_states");
  return FS_EINVAL;
}

void mi_last_timing(double* ms4) {
  for (int k = 0; k < 4; k++) ms4[k] = g_mi_ms[k];
}

int mi_matrices(int device, const uint8_t* codes, const uint8_t* ycodes, int64_t n, int64_t p,
                int n_states, int unit, double* relevance, double* redundancy,
                int32_t* counts_out) {
  if (device_count() <= 0) return no_device();
  for (double& v : g_mi_ms) v = -1.0;
  MiPlanes pl;
  const int T = 16 / ((n_states + 3) / 4);  // columns of a tile's side
  FS_TRY(pl.shape("fs_mi_matrices", n, p, n_states, T));
  const int S = pl.S;
  if ((redundancy && (double)p * (double)p * 8.0 > kMiMaxBytes) ||
      (counts_out && (double)p * (double)p * (double)S * S * 4.0 > kMiMaxBytes)) {
    set_error("fs_mi_matrices: the matrices do not fit the device memory");
    return FS_EOOM;
  }
  const size_t nred = redundancy ? (size_t)p * p : 0;
  const size_t ncnt = counts_out ? (size_t)p * p * S * S : 0;

  FS_HIP(hipSetDevice(device));
  DevArena mem(device);
  StreamLease lease(device);  // destroyed (and the stream synchronised) before `mem`
  FS_TRY(lease.open(5));
  hipStream_t s = lease.s;
  std::vector<hipEvent_t>& ev = lease.ev;
  int32_t* dcnt = nullptr;
  double *dred = nullptr, *drel = nullptr;
  // every block is allocated before any array is read
  FS_TRY(pl.alloc(mem, mem));
  FS_TRY(mem.alloc(&drel, (size_t)p));
  if (nred) FS_TRY(mem.alloc(&dred, nred));
  if (ncnt) FS_TRY(mem.alloc(&dcnt, ncnt));

  FS_HIP(hipEventRecord(ev[0], s));
  FS_TRY(pl.upload(codes, ycodes, s));
  // the diagonal, and every cell of counts_out that no pair writes, stay zero
  if (nred) FS_HIP(hipMemsetAsync(dred, 0, nred * 8, s));
  if (ncnt) FS_HIP(hipMemsetAsync(dcnt, 0, ncnt * 4, s));
  FS_HIP(hipEventRecord(ev[1], s));
  FS_TRY(pl.pack(s));
  FS_HIP(hipEventRecord(ev[2], s));
  FS_TRY(pl.fetch_bad(s));
  FS_HIP(hipStreamSynchronize(s));
  FS_TRY(pl.check());

  // launches of about 2e11 lane operations each (a few milliseconds at the
  // VALU peak), so that no launch holds the device for long: per tile and
  // word 256 lanes run 16 ANDs and 16 popcount-accumulates
  MiScanArgs a;
  a.planes = pl.planes, a.kcol = pl.kcol, a.n = n, a.p = p, a.P1p = pl.P1p, a.W = pl.W;
  a.S = S, a.SP = pl.SP, a.NB = pl.NB, a.T = T, a.nbt = pl.P1p / T, a.unit = unit;
  a.only_y = nred == 0 && ncnt == 0;
  a.red = dred, a.rel = drel, a.counts = dcnt;
  const int64_t tiles = a.only_y ? a.nbt : a.nbt * (a.nbt + 1) / 2;
  const double ops = 256.0 * 32.0 * (double)pl.W;
  int64_t per = (int64_t)std::max(1024.0, std::min(2e11 / ops, 1e9));
  if (test_hooks().mi_tiles > 0) per = test_hooks().mi_tiles;
  for (int64_t t0 = 0; t0 < tiles; t0 += per) {
    a.t0 = t0;
    k_mi_scan<<<(unsigned)std::min<int64_t>(per, tiles - t0), kPtThreads, 0, s>>>(a);
    FS_TRY(launch_check("k_mi_scan"));
  }
  FS_HIP(hipEventRecord(ev[3], s));
  FS_HIP(hipMemcpyAsync(relevance, drel, (size_t)p * 8, hipMemcpyDeviceToHost, s));
  if (nred) FS_HIP(hipMemcpyAsync(redundancy, dred, nred * 8, hipMemcpyDeviceToHost, s));
  if (ncnt) FS_HIP(hipMemcpyAsync(counts_out, dcnt, ncnt * 4, hipMemcpyDeviceToHost, s));
  FS_HIP(hipEventRecord(ev[4], s));
  FS_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < 4; k++) {
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) g_mi_ms[k] = ms;
  }
  (void)hipGetLastError();
  return FS_OK;
}

}  // namespace gpu
}  // namespace fs
