"""Inputs and a float64 restatement for the exact pass-2 tests (numpy only).

Pass 2 sums ``w_ij * |xs_i - xs_j|`` per feature in float32 partials that are
folded into float64.  On data built here every such term and every partial
sum is an exact dyadic number, so the float64 sums the library returns must
equal a numpy float64 sum bit for bit, in whatever order they were added:

* every continuous value is ``k / 64`` with k in 0..64, and rows 0 and 1 are
  all 0 and all 1, so each column has min 0, max 1 and ``recip == 1``: the
  pass-2 operand ``f32((x - min) * recip)`` is x itself and every per-feature
  diff a multiple of 1/64 (a discrete diff is 0 or 1);
* the near / far decisions are the caller's: ``fs_plan_select`` takes row i's
  threshold from ``rowstats[3i..3i+2] = (0, 0, -thr_i * SC * (n - 1))``
  (``rowstats``), and every threshold used here lies at least 1/128 (scaled
  units) from every distance of its row, far outside any quantisation band;
* the counts given to ``fs_plan_pass2`` are powers of two (``counts_pow2``),
  so a pair weight is a multiple of 1/8 of magnitude at most 2.

``check_exactness`` asserts all of this from numpy alone; it is what entitles
a test to ``np.array_equal`` instead of a tolerance.
"""
import numpy as np

GRID = 64
TILE = 128          # pair tile edge
HALF = 64           # rows of a tile half
WAVES = 16          # waves of a sparse pass-2 workgroup: column jj = wave + 16 c
ALL, NONE = 1e6, -1.0


# ---- data -------------------------------------------------------------------

def slot_pairs(n):
    """Disjoint pairs (i, j), i < j, whose weight slots W[t][h][w][r][c]
    (row i % 128 = 64 h + r, column j % 128 = w + 16 c) cover, as far as n
    allows, r in {0, 63}, both halves, wave 0 and 15, c in {0, 7}, a diagonal
    and an off-diagonal tile and the last, partial row block.  Row j never is
    row 0 or 1 (they pin the column ranges) and no row is used twice."""
    last0 = (n - 1) // TILE * TILE
    cand = [(0, 15), (63, 112), (127, 143), (64, 240), (192, 255), (191, 256), (128, 383),
            (63, 64), (126, n - 1), (last0, last0 + 15), (last0 - 1, last0 + 1)]
    used, out = {1}, []
    for i, j in cand:
        if not (0 <= i < j < n) or j < 2 or i in used or j in used:
            continue
        used.update((i, j))
        out.append((i, j))
    return out


def slot_of(i, j):
    """(row block, column block, half, row of the half, wave, column of the wave)."""
    ii, jj = i % TILE, j % TILE
    return i // TILE, j // TILE, ii // HALF, ii % HALF, jj % WAVES, jj // WAVES


def grid_data(n, p, n_discrete, seed, classes=2, pairs=()):
    """(X float32 [n, p], y int64 [n], is_discrete uint8 [p], recip float32 [p]).

    The leading p - n_discrete columns hold k / 64, the trailing n_discrete
    ones codes 0..2; rows 0 and 1 are all 0 and all 1.  For each (i, j) of
    ``pairs`` row j is a copy of row i with one feature moved by one step
    (1/64, or one code where every column is discrete) and row i's label."""
    rng = np.random.default_rng(seed)
    pc = p - n_discrete
    X = np.empty((n, p), dtype=np.float32)
    X[:, :pc] = rng.integers(0, GRID + 1, size=(n, pc)).astype(np.float32) / GRID
    X[:, pc:] = rng.integers(0, 3, size=(n, n_discrete)).astype(np.float32)
    X[0, :] = 0.0
    X[1, :] = 1.0
    y = rng.integers(0, classes, size=n)
    y[:classes] = np.arange(classes)
    for k, (i, j) in enumerate(pairs):
        assert j > 1 and i != j
        X[j] = X[i]
        y[j] = y[i]
        if pc:
            f = k % pc
            X[j, f] += (1.0 if X[i, f] < 1.0 else -1.0) / GRID
        else:
            f = k % p
            X[j, f] = (X[i, f] + 1.0) % 3.0
    isd = np.zeros(p, dtype=np.uint8)
    isd[pc:] = 1
    return X, y, isd, np.ones(p, dtype=np.float32)


def feature_blocks(p, n_discrete):
    """The feature blocks pass 2 cuts the padded layout into, restated from
    fs_prep.cpp (continuous columns first, each kind padded to a multiple of
    64) and fs_pass2.hip: ``sparse`` lists (F, kind) per block of the sparse
    score kernel (512-wide F = 8 blocks, then a tail of at most 256 features
    in one F = 4 block), ``dense`` the kind per 128-wide block of the dense
    one.  kind is "cont" (the generated statement on the sparse route),
    "disc", or "mixed": continuous and discrete lanes in one block."""
    pc = p - n_discrete
    PC, PD = -(-pc // 64) * 64, -(-n_discrete // 64) * 64
    PW = PC + PD

    def kind(f0, f_end):
        return "cont" if f_end <= PC else "disc" if f0 >= PC else "mixed"

    nfb8 = PW // 512 + (PW % 512 > 256)
    f_tail = min(nfb8 * 512, PW)
    sparse = [(8, kind(f0, min(f0 + 512, PW))) for f0 in range(0, f_tail, 512)]
    sparse += [(4, kind(f0, min(f0 + 256, PW))) for f0 in range(f_tail, PW, 256)]
    dense = [kind(f0, min(f0 + 128, PW)) for f0 in range(0, PW, 128)]
    return dict(PC=PC, PW=PW, sparse=sparse, dense=dense)


def counts_pow2(n, tiny=False):
    """(H, M) with H_i = 2^(i % 4) and M_i = 2^((i // 4) % 4).  ``tiny``: the
    rows i % 5 == 2 get H = 2^200, whose hit weight -2^-200 is -0.0 as a
    float: such hits must add nothing to a sum or to weighted_pairs.  (Which
    zero pass 2 stores cannot be seen from its results: a stored -0.0 would
    add |a - b| * -0.0 and change no bit.)"""
    i = np.arange(n)
    H = np.ldexp(1.0, i % 4)
    M = np.ldexp(1.0, (i // 4) % 4)
    if tiny:
        H[i % 5 == 2] = np.ldexp(1.0, 200)
    return H, M


def pack_counts(H, M):
    return np.ascontiguousarray(np.stack([H, M], axis=1).reshape(-1), dtype=np.float64)


def rowstats(thr, SC, n):
    """The rowstats vector from which fs_plan_select derives exactly ``thr``
    (k_thr_ms: thr = (rs0 - rs2) / (n - 1) - sqrt(var) / 2, integer units)."""
    rs = np.zeros(3 * n, dtype=np.float64)
    rs[2::3] = -np.asarray(thr, dtype=np.float64) * SC * (n - 1)
    return rs


# ---- the restatement ----------------------------------------------------------

def _codes(x, isd):
    isd = np.asarray(isd).astype(bool)
    xc = np.asarray(x, dtype=np.float64)[:, ~isd]
    k = np.rint(xc * GRID).astype(np.int64)
    return k, np.asarray(x, dtype=np.float64)[:, isd].astype(np.int64)


def _thermo(k):
    """float32 [n, pc * 64]: T[i, f * 64 + t] = [k_if > t], so that
    64 |x_if - x_jf| = sum_t T_it + T_jt - 2 T_it T_jt."""
    n, pc = k.shape
    return (k[:, :, None] > np.arange(GRID)[None, None, :]).reshape(n, pc * GRID).astype(np.float32)


def _onehot(c):
    n, pd = c.shape
    return (c[:, :, None] == np.arange(3)[None, None, :]).reshape(n, pd * 3).astype(np.float32)


def distances(x, isd):
    """float64 [n, n]: sum |x_i - x_j| over the continuous columns plus the
    number of differing discrete codes.  float32 matrix products of 0 / 1
    values whose sums stay below 2^24: exact."""
    k, c = _codes(x, isd)
    n = k.shape[0]
    assert 2 * GRID * max(k.shape[1], 1) < 2 ** 24 and c.shape[1] < 2 ** 24
    D = np.zeros((n, n), dtype=np.float64)
    if k.shape[1]:
        T = _thermo(k)
        s = T.sum(1, dtype=np.float64)
        D += (s[:, None] + s[None, :] - 2.0 * (T @ T.T).astype(np.float64)) / GRID
    if c.shape[1]:
        O = _onehot(c)
        D += c.shape[1] - (O @ O.T).astype(np.float64)
    np.fill_diagonal(D, 0.0)
    return D


def distances_direct(x, isd):
    """The same from the definition (small shapes: an n x n x p array)."""
    isd = np.asarray(isd).astype(bool)
    x = np.asarray(x, dtype=np.float64)
    d = np.abs(x[:, None, :] - x[None, :, :])
    return d[:, :, ~isd].sum(-1) + (d[:, :, isd] != 0).sum(-1)


def _weighted_sums(x, isd, W32):
    """float64 [p]: sum_{i<j} W32_ij d_f(i, j) for a symmetric float32 weight
    matrix of multiples of 1/8 with a zero diagonal, without an n x n x p
    array: through the 64 steps (3 codes) of a column."""
    k, c = _codes(x, isd)
    n = W32.shape[0]
    wmax = float(np.abs(W32).max()) if W32.size else 0.0
    assert 8 * wmax * n < 2 ** 24, "float32 products would not be exact"
    rowsum = W32.sum(1, dtype=np.float64)
    isd = np.asarray(isd).astype(bool)
    out = np.zeros(isd.size, dtype=np.float64)
    if k.shape[1]:
        T = _thermo(k)
        R = rowsum[:, None] - (W32 @ T).astype(np.float64)
        lev = (T * R).sum(0, dtype=np.float64)
        out[~isd] = lev.reshape(k.shape[1], GRID).sum(1) / GRID
    if c.shape[1]:
        O = _onehot(c)
        same = (O * (W32 @ O).astype(np.float64)).sum(0, dtype=np.float64)
        out[isd] = 0.5 * rowsum.sum() - 0.5 * same.reshape(c.shape[1], 3).sum(1)
    return out


def weighted_sums_direct(x, isd, W32):
    """The same from the definition (small shapes)."""
    isd = np.asarray(isd).astype(bool)
    x = np.asarray(x, dtype=np.float64)
    d = np.abs(x[:, None, :] - x[None, :, :])
    d[:, :, isd] = d[:, :, isd] != 0
    return 0.5 * np.einsum("ij,ijf->f", W32.astype(np.float64), d)


def _focal(n, rows):
    f = np.zeros(n, dtype=bool)
    lo, hi = (0, n) if rows is None else rows
    f[lo:hi] = True
    return f


def _result(x, isd, near, hit, W, rows):
    n = near.shape[0]
    W = np.where(_focal(n, rows)[:, None], W, 0.0)
    np.fill_diagonal(W, 0.0)
    with np.errstate(under="ignore"):
        W32 = (W + W.T).astype(np.float32)      # pair_weight: (float)(w_i + w_j)
    W32[W32 == 0] = 0.0                         # -0.0 is no weight
    return dict(near=near, hits=(near & hit).sum(1).astype(np.float64),
                misses=(near & ~hit).sum(1).astype(np.float64),
                weighted=int(np.count_nonzero(np.triu(W32, 1))), W32=W32,
                sums=_weighted_sums(x, isd, W32))


def expected(x, y, isd, thr, H, M, use_star, rows=None, D=None):
    """MultiSURF / MultiSURF* pass 2 in float64 for the decisions
    ``D_ij < thr_i`` and the counts (H, M): a dict with ``D``, ``near``, the
    near ``hits`` / ``misses`` per row, ``weighted`` (pairs i < j with a
    non-zero weight), the float32 pair weights ``W32`` and ``sums`` [p].
    W_ij is multisurf_weight (fs_internal.h): near hit -1 / H_i, near miss
    1 / M_i, far miss (star) -1 / max(M_i, 1); ``rows`` = (lo, hi) keeps the
    focal rows of fs_plan_set_rows."""
    if D is None:
        D = distances(x, isd)
    n = D.shape[0]
    y = np.asarray(y)
    off = ~np.eye(n, dtype=bool)
    hit = (y[:, None] == y[None, :]) & off
    near = (D < np.asarray(thr, dtype=np.float64)[:, None]) & off
    H = np.asarray(H, dtype=np.float64)[:, None]
    M = np.asarray(M, dtype=np.float64)[:, None]
    W = np.where(near, np.where(hit, -1.0 / H, 1.0 / M), 0.0)
    if use_star:
        W = np.where(~near & ~hit & off, -1.0 / np.maximum(M, 1.0), W)
    r = _result(x, isd, near, hit, W, rows)
    r["D"] = D
    return r


SURF_MARGIN = 1e-4


def surf_expected(x, y, isd, use_star, rows=None, D=None):
    """SURF / SURF* in float64.  The threshold of row i is the reference's:
    the float32 sequential sum of its float32 distances over n - 1.  Both are
    exact here (asserted), and no distance lies within SURF_MARGIN of its
    row's mean (asserted), so no decision rests on the mean's last bit."""
    if D is None:
        D = distances(x, isd)
    n, p = D.shape[0], np.asarray(x).shape[1]
    assert p * GRID < 2 ** 24 and D.sum(1).max() * GRID < 2 ** 24
    avg = D.sum(1) / (n - 1)
    off = ~np.eye(n, dtype=bool)
    gap = np.abs(D - avg[:, None])[off].min()
    assert gap > SURF_MARGIN, f"a distance {gap:.2e} from its row mean: pick another seed"
    y = np.asarray(y)
    hit = (y[:, None] == y[None, :]) & off
    near = (D < avg[:, None]) & off
    W = np.where(near, np.where(hit, -1.0, 1.0), 0.0)
    if use_star:
        W = np.where(~near & off, np.where(hit, 1.0, -1.0), W)
    r = _result(x, isd, near, hit, W, rows)
    r["D"] = D
    return r


# ---- thresholds -----------------------------------------------------------------

def _quantile_thr(D, q):
    n = D.shape[0]
    S = np.sort(D + np.diag(np.full(n, np.inf)), axis=1)[:, :n - 1]
    return S[:, int(q * (n - 1))] + 0.5 / GRID


def patterns(D, n, pairs=(), rows=(0, 63, 64, 127, 128, -1)):
    """Named threshold vectors (scaled units), each at a multiple of 1/64 plus
    1/128: ``none`` / ``all``, each row's own 1 % / 40 % / 99 % distance
    quantile, ``even`` rows all near, ``half0`` (rows i % 128 < 64 all near),
    ``row(i)`` one focal row alone, ``pair(i,j)`` one pair alone (``pairs``
    as given to grid_data)."""
    i = np.arange(n)
    out = {"none": np.full(n, NONE), "all": np.full(n, ALL)}
    for q in (1, 40, 99):
        out[f"q{q:02d}"] = _quantile_thr(D, q / 100.0)
    out["even"] = np.where(i % 2 == 0, ALL, NONE)
    out["half0"] = np.where(i % TILE < HALF, ALL, NONE)
    for r in sorted({r % n for r in rows if -n <= r < n}):
        out[f"row({r})"] = np.where(i == r, ALL, NONE)
    for a, b in pairs:
        t = np.full(n, NONE)
        t[a] = D[a, b] + 0.5 / GRID
        assert ((D[a] < t[a]) & (i != a)).sum() == 1, f"pair({a},{b}) is not alone"
        out[f"pair({a},{b})"] = t
    return out


def check_exactness(x, isd, D, thr, H, M, W32):
    """The preconditions of bit equality, from numpy alone."""
    isd = np.asarray(isd).astype(bool)
    xc = np.asarray(x, dtype=np.float64)[:, ~isd]
    k = xc * GRID
    assert np.array_equal(k, np.rint(k)) and k.min(initial=0) >= 0 and k.max(initial=0) <= GRID
    if xc.shape[1]:
        assert np.all(xc.min(0) == 0.0) and np.all(xc.max(0) == 1.0)
    for v in (H, M):
        m, _ = np.frexp(np.asarray(v, dtype=np.float64))
        assert np.all(m == 0.5), "a count that is no power of two"
    w = np.abs(np.asarray(W32, dtype=np.float64))
    assert np.array_equal(w * 8, np.rint(w * 8))
    # a float32 partial of up to 1024 terms, each a multiple of 1 / (64 * 8)
    assert 1024 * w.max(initial=0.0) * GRID * 8 < 2 ** 24
    n = D.shape[0]
    gap = np.abs(D - np.asarray(thr, dtype=np.float64)[:, None])[~np.eye(n, dtype=bool)]
    assert gap.min() >= 0.5 / GRID, "a threshold closer than 1/128 to a distance"


# ---- driving a plan ---------------------------------------------------------------

class HostBufs:
    """The exchange vectors of a CPU plan (numpy host memory)."""

    def __init__(self, n, p):
        self.n, self.p = n, p
        self.rs = np.zeros(3 * n)
        self.sel = np.zeros(2 * n)
        self.cnt = np.zeros(2 * n)
        self.sc = np.zeros(p)

    def put(self, name, v):
        getattr(self, name)[:] = v

    def get(self, name):
        return getattr(self, name).copy()

    def ptr(self, name):
        return getattr(self, name).ctypes.data

    def sync(self):
        pass


class DevBufs:
    """The exchange vectors of a GPU plan (torch device memory; torch is
    imported here, by the GPU tests alone)."""

    def __init__(self, n, p):
        import torch
        self.n, self.p, self.torch = n, p, torch
        dev = torch.device("cuda", 0)
        self.t = {k: torch.zeros(m, dtype=torch.float64, device=dev)
                  for k, m in (("rs", 3 * n), ("sel", 2 * n), ("cnt", 2 * n), ("sc", p))}
        self.sync()

    def put(self, name, v):
        self.t[name].copy_(self.torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)))

    def get(self, name):
        return self.t[name].cpu().numpy()

    def ptr(self, name):
        return self.t[name].data_ptr()

    def sync(self):
        self.torch.cuda.synchronize()  # the plan runs on its own stream


def select_and_score(plan, bufs, thr, counts, SC):
    """One select on the caller's thresholds, one pass 2 on the caller's
    counts: (near hit / miss counts [n, 2] from select, float64 sums)."""
    bufs.put("rs", rowstats(thr, SC, bufs.n))
    bufs.put("cnt", counts)
    bufs.put("sc", np.full(bufs.p, np.nan))   # pass 2 must write every score
    bufs.sync()
    plan.select(bufs.ptr("rs"), bufs.ptr("sel"))
    plan.pass2(bufs.ptr("cnt"), bufs.ptr("sc"))
    bufs.sync()
    return bufs.get("sel").reshape(-1, 2), bufs.get("sc")
