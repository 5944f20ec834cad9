"""fs_pair_screen_labels on the GPU (fs_pairscan_labels.hip, k_pair_lab).

The identity that pins the kernels, without a tolerance: row b equals the GPU's
own pair_screen(codes, labels[b], n_top=1) on score, pair and relevance.

Shapes are the smallest at which the kernels can go wrong.  Up to 4 states a
lane is a labelling and a wave takes one pair at a time, four waves a block on
interleaved ranks of the block's run; the planes and the labels are laid out in
quads of four words (128 samples):

* lanes: B = 1, 63, 64, 65, 130 (one ragged wave, one full, a second block row
  of one lane, three), row 0 the data's y, the others permutations, one
  duplicate row and one one-class row;
* pairs: p = 2 (one pair, three idle waves), 3, 9 (36 pairs: every wave of a
  block gets several) and 41 (820 pairs);
* words: n = 33, 64, 129 and 2049 (a ragged and a full quad, two quads and a
  word, 17 quads);
* states 2, 3, 4 x classes 2, 3, 4, with columns of fewer states than the
  plane count (zero cells), tied() (runs of equal keys: the smaller rank must
  win across waves and blocks) and all_constant();
* the general route: 5 states x 2 classes at p = 9, B = 3, and 32 states x 4
  classes at p = 3, n = 257, B = 2;
* launch splits at p = 41, B = 130: three label chunks, four rank chunks, and
  both; each test first asserts by arithmetic that the split happens.

Against the CPU backend the best scores agree within TOL = 1e-10 (the rule of
test_gpu_pairscan.py), and the pair is equal wherever the CPU's best exceeds its
runner-up by more than 2 TOL.
"""
import numpy as np
import pytest

import mi_np
import pairscan_np

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCORES = ("joint", "gain")
WAVES = 4              # kPlWaves: the waves of a block


@pytest.fixture(scope="module")
def L():
    from fastselect_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    return _lib


def _labels(y, B, seed):
    """Row 0 is y, the others permutations; from four rows on, row 2 repeats
    row 1 and row 3 is a single class."""
    rng = np.random.default_rng(seed)
    lab = np.stack([y] + [rng.permutation(y) for _ in range(B - 1)]).astype(np.uint8)
    if B >= 4:
        lab[2] = lab[1]
        lab[3] = 0
    return lab


def _u(n, p, states, seed, classes, B):
    def make():
        X, y = mi_np.uniform(n, p, states, seed, classes)
        return X, _labels(y, B, seed + 1), max(states, classes)
    return make


def _fewer_states(classes):
    """Four planes; the columns take 1..4 states."""
    def make():
        rng = np.random.default_rng(600 + classes)
        X = np.stack([rng.integers(0, 1 + f % 4, 97) for f in range(9)], axis=1).astype(np.uint8)
        y = rng.integers(0, classes, 97)
        return X, _labels(y, 5, 610 + classes), 4
    return make


def _from(case, B, seed):
    def make():
        X, y, S = case()
        return X, _labels(y, B, seed), S
    return make


def _classes_differ():
    """Rows of two, three and four classes in one batch of common count 4."""
    X, y = mi_np.uniform(97, 9, 3, 640, 4)
    lab = _labels(y, 6, 641)
    lab[4] = lab[4] % 2
    lab[5] = np.minimum(lab[5], 2)
    return X, lab, 4


SHAPES = {}
for _B in (1, 63, 64, 65, 130):
    SHAPES["B%d" % _B] = _u(65, 9, 3, 500 + _B, 2, _B)
for _p in (2, 3, 9, 41):
    SHAPES["p%d" % _p] = _u(65, _p, 3, 520 + _p, 2, 5)
for _n in (33, 64, 129, 2049):
    SHAPES["n%d" % _n] = _u(_n, 9, 3, 540 + _n, 3, 5)
for _s in (2, 3, 4):
    for _c in (2, 3, 4):
        SHAPES["s%d_c%d" % (_s, _c)] = _u(97, 9, _s, 560 + 10 * _s + _c, _c, 5)
for _c in (2, 3, 4):
    SHAPES["fewer_states_c%d" % _c] = _fewer_states(_c)
SHAPES.update({
    "classes_differ": _classes_differ,
    "tied": _from(pairscan_np.tied, 5, 650),
    "tied_B70": _from(pairscan_np.tied, 70, 651),
    "all_constant": _from(pairscan_np.all_constant, 5, 652),
    "general_s5_c2": _u(65, 9, 5, 660, 2, 3),
    "general_s32_c4": _u(257, 3, 32, 661, 4, 2),
    "split": _u(65, 41, 3, 670, 2, 130),
})

_DATA = {}


def _data(L, name, score):
    """(X, labels, S, the GPU's single calls row by row: score, pair, relevance)."""
    if (name, score) not in _DATA:
        X, labels, S = SHAPES[name]()
        X = np.ascontiguousarray(X, dtype=np.uint8)
        singles = {}
        best, pairs, rels = [], [], []
        for b in range(labels.shape[0]):
            key = labels[b].tobytes()      # equal rows: one call
            if key not in singles:
                r, s, pr, _ = L.pair_screen("gpu", X, labels[b], S, n_top=1, score=score,
                                            want_feature_best=False)
                singles[key] = (s[0], pr[0], r)
            s, pr, r = singles[key]
            best.append(s), pairs.append(pr), rels.append(r)
        want = (np.array(best), np.array(pairs), np.array(rels))
        for a in (X, labels) + want:
            a.setflags(write=False)
        _DATA[(name, score)] = (X, labels, S, want)
    return _DATA[(name, score)]


def _assert_identical(got, want):
    for g, w, what in zip(got, want, ("score", "pair", "relevance")):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        bad = np.argwhere(g != w)
        assert np.array_equal(g, w), (what, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert not np.signbit(got[0]).any()


@pytest.mark.parametrize("score", SCORES)
@pytest.mark.parametrize("name", sorted(set(SHAPES) - {"split"}))
def test_rows_are_the_single_calls(L, name, score):
    X, labels, S, want = _data(L, name, score)
    got = L.pair_screen_labels("gpu", X, labels, S, score=score, want_relevance=True)
    _assert_identical(got, want)
    if labels.shape[0] >= 4:               # the one-class row
        assert got[0][3] == 0.0 and tuple(got[1][3]) == (0, 1) and not got[2][3].any()
    if name == "all_constant":
        assert not got[0].any() and (got[1] == (0, 1)).all() and not got[2].any()


def test_relevance_is_optional(L):
    X, labels, S, want = _data(L, "p9", "gain")
    best, pairs, rel = L.pair_screen_labels("gpu", X, labels, S, score="gain")
    assert rel is None
    assert np.array_equal(best, want[0]) and np.array_equal(pairs, want[1])


@pytest.mark.parametrize("hooks", [{"pair_labels": 64}, {"pair_lab_ranks": 256},
                                   {"pair_labels": 64, "pair_lab_ranks": 256},
                                   {"pair_labels": 100, "pair_lab_ranks": 7}],
                         ids=["labels", "ranks", "both", "odd"])
def test_launch_splits_change_no_bit(L, hooks):
    X, labels, S, want = _data(L, "split", "gain")
    B, pairs = labels.shape[0], X.shape[1] * (X.shape[1] - 1) // 2
    assert (B, pairs) == (130, 820)
    if "pair_labels" in hooks:
        chunk = max(64, hooks["pair_labels"] // 64 * 64)
        assert chunk == 64 and -(-B // chunk) == 3          # b0 = 0, 64, 128
    if "pair_lab_ranks" in hooks:
        assert -(-pairs // hooks["pair_lab_ranks"]) >= 3
    unsplit = L.pair_screen_labels("gpu", X, labels, S, score="gain", want_relevance=True)
    with L.test_hooks(**hooks):
        got = L.pair_screen_labels("gpu", X, labels, S, score="gain", want_relevance=True)
    _assert_identical(got, unsplit)
    _assert_identical(got, want)


@pytest.mark.parametrize("score", SCORES)
@pytest.mark.parametrize("name", ["B65", "p41", "n2049", "s4_c4", "fewer_states_c3",
                                  "classes_differ", "general_s5_c2"])
def test_against_the_cpu_backend(L, name, score):
    X, labels, S, _ = _data(L, name, score)
    best, pairs, rel = L.pair_screen_labels("gpu", X, labels, S, score=score, want_relevance=True)
    cbest, cpairs, crel = L.pair_screen_labels("cpu", X, labels, S, score=score,
                                               want_relevance=True)
    assert np.abs(best - cbest).max() <= TOL
    assert np.abs(rel - crel).max() <= TOL
    for b in range(labels.shape[0]):
        _, s2, _, _ = L.pair_screen("cpu", X, labels[b], S, n_top=2, score=score,
                                    want_feature_best=False)
        if s2.size < 2 or s2[0] - s2[1] > 2 * TOL:
            assert tuple(pairs[b]) == tuple(cpairs[b]), b


def test_estimator_on_the_planted_pair(L):
    from fastselect_amd import PairScreen
    X, y = pairscan_np.pure(400, 20, 11, 7, 13, 2)
    t = PairScreen(4, n_top=12, backend="gpu").permutation_test(X, y, 99, random_state=5)
    assert t.effective_backend_ == "gpu"
    assert tuple(t.top_pairs_[0]) == (7, 13)
    assert t.p_value_ == 0.01
    assert t.null_max_scores_.shape == (99,) and t.null_max_scores_.max() < 0.05
    assert np.all(np.diff(t.top_p_values_) >= 0.0) and t.top_p_values_[0] == t.p_value_


def test_timing(L):
    X, labels, S, _ = _data(L, "p9", "gain")
    L.pair_screen_labels("gpu", X, labels, S)
    ms = L.pair_labels_last_timing()
    assert len(ms) == 5 and all(t >= 0.0 for t in ms)
