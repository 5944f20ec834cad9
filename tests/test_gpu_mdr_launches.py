"""The launch splits of the three MDR entry points on the GPU (fs_mdr.hip).

fs_mdr_scan, fs_mdr_scan_top and fs_mdr_scan_labels split C(p,k) into launches
of about 2e11 lane operations with a floor of 65536 ranks, give a launch at
most 2048 (labels: 1024) blocks, and the labels scan splits its labellings too.
At the sizes a test can compare in full none of this happens, so three test
hooks shrink the constants (0 = the product's own arithmetic):

* ``mdr_ranks``   ranks per launch, without the floor: several launches, whose
  block slots merge, whose histogram and candidate cursor accumulate and whose
  ``ba_out`` is written at r0 > 0;
* ``mdr_blocks``  blocks per launch: a block's run exceeds one step, so a lane
  steps its combination by 256 (labels: a wave by 4) with mdr_advance, across
  the row ends of the combination triangle;
* ``mdr_labels``  labellings per launch: label chunks with b0 > 0.

Everything is compared bit for bit with the CPU backend and the numpy
restatement: all quantities are integers until three float64 operations.
Every test first asserts, in Python arithmetic from the hook values, that its
shape takes the route it is about (``route`` / ``labels_route`` restate the
launch arithmetic of fs_mdr.hip)."""
import numpy as np
import pytest

import mdr_np
from mdr_top_np import expected, same, same_bits

pytestmark = pytest.mark.gpu

THREADS = 256        # kMdrThreads
MAX_BLOCKS = 2048    # kMdrMaxBlocks
LAB_WAVES = 4        # kMdrLabWaves
LAB_MAX_BLOCKS = 1024
BIN_SHIFT, BIN_BASE, BINS = 14, 0x3F000000 >> 14, 514


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


def ceil_div(a, b):
    return -(-a // b)


def route(count, ranks=0, blocks=0):
    """(launches, steps): the rank launches of one scan of `count` ranks and
    the 256-rank steps a block of the first launch takes.  The product's own
    chunk is at least 65536 ranks, above every count used here."""
    assert count < 65536
    chunk = ranks if ranks > 0 else count
    first = min(count, chunk)
    nblocks = min(blocks if blocks > 0 else MAX_BLOCKS, ceil_div(first, THREADS))
    return ceil_div(count, chunk), ceil_div(first, nblocks * THREADS)


def labels_route(count, B, ranks=0, blocks=0, labels=0):
    """(rank launches, steps of a wave in the first one, label chunks)."""
    assert count < 4096   # the product's own rank chunk is above 15000 at the sizes used here
    chunk = ranks if ranks > 0 else count
    first = min(count, chunk)
    runs = ceil_div(first, LAB_WAVES)
    nblocks = min(blocks if blocks > 0 else LAB_MAX_BLOCKS, runs)
    lab_chunk = max(64, labels // 64 * 64) if labels > 0 else ceil_div(B, 64) * 64
    return ceil_div(count, chunk), ceil_div(runs, nblocks), ceil_div(B, lab_chunk)


def hook_args(ranks=0, blocks=0, labels=0, cap=0):
    h = {"mdr_ranks": ranks, "mdr_blocks": blocks, "mdr_labels": labels, "mdr_top_cap": cap}
    return {k: v for k, v in h.items() if v > 0}


def comb(p, k):
    c = 1
    for i in range(k):
        c = c * (p - i) // (i + 1)
    return c


# ---- fs_mdr_scan -------------------------------------------------------------
# The parity shapes of test_gpu_mdr.py (C(p,k) = 126, 7, 364, 780), and k = 4,
# 5, 6 at p = 11 (330, 462, 462): a count above 256, so that one block takes a
# second step and mdr_advance(256) runs for every k from 2 to 6.
SCAN_SHAPES = [(97, 9, 4, 2), (50, 7, 6, 2), (203, 14, 3, 3), (203, 40, 2, 5),
               (97, 11, 4, 2), (97, 11, 5, 2), (97, 11, 6, 2)]
# (ranks per launch, blocks per launch): singly and together.  100 is no
# multiple of 256; 3 splits the 7 combinations of (50, 7, 6, 2); 300 ranks with
# one block and 600 with two are several launches of two steps each.
SCAN_HOOKS = [(100, 0), (256, 0), (3, 0), (0, 1), (0, 2), (300, 1), (600, 2)]


def takes_route(count, ranks, blocks):
    """Every hook that is set changes the launches: more ranks than one launch
    holds, and more ranks in a launch than its blocks take in one step."""
    launches, steps = route(count, ranks, blocks)
    return (not ranks or (count > ranks and launches > 1)) and \
        (not blocks or (min(count, ranks or count) > blocks * THREADS and steps > 1))


def scan_cases():
    """Every (shape, hooks) pair whose hooks all take effect (the test asserts
    it again)."""
    return [(n, p, k, cv, ranks, blocks) for n, p, k, cv in SCAN_SHAPES
            for ranks, blocks in SCAN_HOOKS if takes_route(comb(p, k), ranks, blocks)]


def test_scan_cases_cover_every_k():
    """Host arithmetic only: for every k from 2 to 6 some case advances a
    combination by 256 and some case takes several launches; some case does
    both at once."""
    adv, split, both = set(), set(), False
    for n, p, k, cv, ranks, blocks in scan_cases():
        launches, steps = route(comb(p, k), ranks, blocks)
        if steps > 1:
            adv.add(k)
        if launches > 1:
            split.add(k)
        both |= steps > 1 and launches > 1
    assert adv >= {2, 3, 4, 5, 6} and split >= {2, 3, 4, 5, 6} and both


def _scan_same(L, X, is_case, k, fold, cv, want, **hooks):
    cb, cr, cba = L.mdr_scan("cpu", X, is_case, k, fold, cv, want_ba=True)
    with L.test_hooks(**hooks):
        gb, gr, gba = L.mdr_scan("gpu", X, is_case, k, fold, cv, want_ba=True)
        gb2, gr2 = L.mdr_scan("gpu", X, is_case, k, fold, cv)
    assert same_bits(gba, cba) and same_bits(gba, want)
    assert same_bits(gb, cb) and np.array_equal(gr, cr)
    assert np.array_equal(gr, np.argmax(want, axis=1)) and same_bits(gb, want.max(axis=1))
    assert same_bits(gb2, gb) and np.array_equal(gr2, gr)
    return gr


@pytest.mark.parametrize("n,p,k,cv,ranks,blocks", scan_cases())
def test_scan_split_equals_cpu_and_numpy(L, n, p, k, cv, ranks, blocks):
    assert takes_route(comb(p, k), ranks, blocks)
    X, y, fold, want = mdr_np.case(n, p, k, cv)
    _scan_same(L, X, y == 1, k, fold, cv, want, **hook_args(ranks, blocks))


@pytest.mark.parametrize("ranks,blocks", [(100, 0), (300, 1), (600, 2)])
def test_scan_two_fold_groups_split(L, ranks, blocks):
    """cv = 20 runs in two groups of folds (16 + 4): the slots merge across
    rank launches x fold groups."""
    n, p, k, cv = 400, 40, 2, 20
    assert cv > 16 and takes_route(comb(p, k), ranks, blocks)
    X, y, fold, want = mdr_np.case(n, p, k, cv)
    _scan_same(L, X, y == 1, k, fold, cv, want, **hook_args(ranks, blocks))


def test_scan_duplicated_column_copies_in_different_launches(L):
    """Column 12 repeats column 5, so (2, 12) ties with the planted (2, 5).  At
    30 ranks per launch the copies' ranks (25 and 32) lie in different launches
    and meet in block 0's slot: the earlier copy must still win."""
    X, y = mdr_np.planted(203, 12, pair=(2, 5))
    X = np.concatenate([X, X[:, 5:6]], axis=1)
    fold, _ = mdr_np.fold_ids(X, y, 3)
    ranks = 30
    ra = [c for c in range(78) if L.mdr_unrank(13, 2, c) == (2, 5)][0]
    rb = [c for c in range(78) if L.mdr_unrank(13, 2, c) == (2, 12)][0]
    assert comb(13, 2) == 78 > ranks and ra // ranks != rb // ranks
    want = mdr_np.scan(X, y == 1, 2, fold, 3)
    assert same_bits(want[:, ra], want[:, rb])
    gr = _scan_same(L, X, y == 1, 2, fold, 3, want, mdr_ranks=ranks)
    assert gr.tolist() == [ra] * 3


# ---- fs_mdr_scan_top ---------------------------------------------------------
TOPS = (1, 7, 300)
TOP_HOOKS = [(100, 0), (256, 0), (0, 1), (0, 2), (300, 1), (600, 2)]
_NOISE = []


def top_data(name):
    """(X, y, k, fold, cv, F x C BAs): the tie case (4060 triples on 16
    samples) or the parity shape (203, 40, 2, 5) (780 pairs, 5 folds)."""
    if name == "noise":
        if not _NOISE:
            X, y = mdr_np.noise_16x30()
            _NOISE.extend((X, y, mdr_np.scan(X, y == 1, 3)))
        X, y, ba = _NOISE
        return X, y, 3, None, 0, ba
    X, y, fold, ba = mdr_np.case(203, 40, 2, 5)
    return X, y, 2, fold, 5, ba


def candidates(ba, n_top):
    """What fs_mdr_scan_top's histogram scan finds: per fold the number of BAs
    in or above the bin (leading bits, mdr_bin of fs_mdr.h) of the n_top-th
    best, summed over the folds.  Above the candidate cap the scan takes the
    bounded-memory route."""
    bits = np.ascontiguousarray(ba, dtype=np.float32).view(np.uint32).astype(np.int64)
    h = bits >> BIN_SHIFT
    b = np.where(h < BIN_BASE, 0, np.minimum(h - BIN_BASE + 1, BINS - 1))
    need = min(n_top, ba.shape[1])
    total = 0
    for f in range(ba.shape[0]):
        kth = np.sort(b[f])[::-1][need - 1]
        total += int(np.sum(b[f] >= kth))
    return total


@pytest.mark.parametrize("n_top", TOPS)
@pytest.mark.parametrize("ranks,blocks", TOP_HOOKS)
@pytest.mark.parametrize("name", ["noise", "parity"])
def test_top_split_equals_cpu_and_numpy(L, name, ranks, blocks, n_top):
    """Both scans split: the histogram accumulates over the launches, and so
    does the candidate cursor."""
    X, y, k, fold, cv, ba = top_data(name)
    assert takes_route(ba.shape[1], ranks, blocks)
    c = L.mdr_scan_top("cpu", X, y == 1, k, fold, cv, n_top=n_top)
    with L.test_hooks(**hook_args(ranks, blocks)):
        g = L.mdr_scan_top("gpu", X, y == 1, k, fold, cv, n_top=n_top)
    assert same(g, c) and same(g, expected(ba, n_top))


# (data, n_top, candidate cap, ranks per launch): the cap is below the
# candidates of that n_top (594 for every n_top on the tie case; 36 and 1534 on
# the parity shape), and a fold's share of it, the ranks one collecting pass
# covers, is above the ranks per launch, so every pass takes several launches.
# The parity shape has 5 candidates at n_top = 1, one per fold: no cap below
# that leaves a pass more than one rank, so that pair is not listed.
TOP_CAPPED = [("noise", 1, 256, 100), ("noise", 7, 256, 100), ("noise", 300, 256, 100),
              ("parity", 7, 30, 3), ("parity", 300, 1000, 100)]


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("name,n_top,cap,ranks", TOP_CAPPED)
def test_top_split_on_the_bounded_memory_route(L, name, n_top, cap, ranks, blocks):
    """A small mdr_top_cap beside the launch hooks: rank chunks of cap / F ranks
    with a running list per fold, each chunk collected in several launches."""
    X, y, k, fold, cv, ba = top_data(name)
    F, count = ba.shape
    assert candidates(ba, n_top) > cap           # the bounded-memory route
    assert count > cap // F > ranks               # several passes of several launches
    c = L.mdr_scan_top("cpu", X, y == 1, k, fold, cv, n_top=n_top)
    with L.test_hooks(**hook_args(ranks, blocks, cap=cap)):
        g = L.mdr_scan_top("gpu", X, y == 1, k, fold, cv, n_top=n_top)
    assert same(g, c) and same(g, expected(ba, n_top))


# ---- fs_mdr_scan_labels ------------------------------------------------------
LAB_B = 130
# (ranks per launch, blocks per launch), singly and together; every case runs
# with 64 labellings per launch: chunks of 64, 64 and 2
LAB_HOOKS = [(4, 0), (10, 0), (0, 1), (0, 3), (10, 1), (10, 2)]
LAB_SHAPES = [(24, 2), (24, 3), (8, 6)]   # (p, k): 276, 2024 and 28 combinations
_LAB = {}


def labels_case(L, p, k, cv):
    """(X, labels, fold, the CPU backend's (best, rank, BAs), the single GPU
    scan of row 0 without hooks), once per session."""
    key = (p, k, cv)
    if key not in _LAB:
        X, y = mdr_np.planted(203, p)
        fold = mdr_np.fold_ids(X, y, cv)[0] if cv else None
        rng = np.random.default_rng(1)
        rows = [(y == 1).astype(np.uint8)]
        rows += [rng.permutation(rows[0]) for _ in range(1, LAB_B)]
        labels = np.stack(rows)
        cpu = L.mdr_scan_labels("cpu", X, labels, k, fold, cv, want_ba=True)
        single = L.mdr_scan("gpu", X, labels[0], k, fold, cv, want_ba=True)
        _LAB[key] = (X, labels, fold, cpu, single)
    return _LAB[key]


@pytest.mark.parametrize("ranks,blocks", LAB_HOOKS)
@pytest.mark.parametrize("cv", [0, 10, 17])
@pytest.mark.parametrize("p,k", LAB_SHAPES)
def test_labels_split_equals_cpu_and_single_scan(L, p, k, cv, ranks, blocks):
    count = comb(p, k)
    launches, steps, chunks = labels_route(count, LAB_B, ranks, blocks, 64)
    assert LAB_B > 64 and chunks == 3
    if ranks:
        assert count > ranks and launches > 1
    if blocks:
        assert min(count, ranks or count) > blocks * LAB_WAVES and steps > 1
    X, labels, fold, (cb, cr, cba), (sb, sr, sba) = labels_case(L, p, k, cv)
    with L.test_hooks(**hook_args(ranks, blocks, labels=64)):
        gb, gr, gba = L.mdr_scan_labels("gpu", X, labels, k, fold, cv, want_ba=True)
        gb2, gr2 = L.mdr_scan_labels("gpu", X, labels, k, fold, cv)
    assert same_bits(gba, cba) and same_bits(gb, cb) and np.array_equal(gr, cr)
    assert same_bits(gb2, gb) and np.array_equal(gr2, gr)
    assert same_bits(gba[0], sba) and same_bits(gb[0], sb) and np.array_equal(gr[0], sr)


def test_labels_cases_cover_every_route():
    """Host arithmetic only: for every k some case steps a wave's combination
    by 4, some case takes several rank launches, and some case does both."""
    adv, split, both = set(), set(), set()
    for p, k in LAB_SHAPES:
        for ranks, blocks in LAB_HOOKS:
            launches, steps, chunks = labels_route(comb(p, k), LAB_B, ranks, blocks, 64)
            assert chunks == 3
            if steps > 1:
                adv.add(k)
            if launches > 1:
                split.add(k)
            if steps > 1 and launches > 1:
                both.add(k)
    assert adv == split == both == {2, 3, 6}
