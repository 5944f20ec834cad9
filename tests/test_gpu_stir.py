"""STIR on the GPU (fs_stir.hip: k_stir_weights + k_stir_score) against the
float64 numpy model (stir_np.py) and against itself.

Sum bar.  Every term of the four sums is non-negative, so nothing cancels:
the relative error of a sum is bounded by that of its terms.  A term is
|a - b| of two float32 pass-2 operands (each rounded once: ~6e-8 of the
feature's range) or its square, put on a fixed-point grid of 2.4e-7 of the
range and summed exactly, so the sums sit well below 1e-6 (seen on an MI355X:
5.2e-8 at most over the four shapes); the assertion is the project's parity
bar, 1e-5, on every entry.  t is held to that bar propagated through the
epilogue (stir_np.t_tolerance).  Sums that regroup the device's own terms
(shards, row ranges, chunks) are held to 1e-12.
"""
import numpy as np
import pytest

import stir_np

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-5
ADD_TOL = 1e-12

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    from fastselect_amd import _lib
    assert _lib.device_count() >= 1, "no HIP device visible: GPU tests cannot run"


# name -> (n, continuous columns, discrete columns)
SHAPES = {
    # three row blocks with a ragged last one, one block half continuous, half discrete
    "mixed": (300, 20, 20),
    # one sample row past a tile; three 128-feature blocks with a ragged tail,
    # the continuous part padded to 256, the last block wholly discrete
    "n130-p270": (130, 200, 70),
    "continuous-p64": (130, 64, 0),
    "discrete-p64": (130, 0, 64),
    # five row blocks (15 tiles, a ragged last block); a two-half continuous
    # feature block and a one-half discrete one: the multi-tile segment walk
    "n600-p140": (600, 100, 40),
}


def case(name):
    """(x, y, recip, isd, model sums, |H|, |M|, model counts), once per session."""
    if name not in _CACHE:
        n, pc, pd = SHAPES[name]
        x, y = stir_np.mixed_case(n, pc, pd)
        recip, isd = stir_np.preprocess(x)
        assert int(isd.sum()) == pd
        _CACHE[name] = (x, y, recip, isd) + stir_np.stir_sums(x, y, recip, isd)
    return _CACHE[name]


def gpu_stir(x, y, recip, isd, feat=None, rows=None, shards=None, accumulation="fast",
             steps_after=0):
    """(sums, |H|, |M|, scores of each step, weighted pairs after each step)
    of one job: step, stir, then ``steps_after`` more steps."""
    from fastselect_amd.parallel import ShardedMultiSURF
    job = ShardedMultiSURF(x, y, recip, isd, backend="gpu", shard=False, rows=rows,
                           shards=shards, accumulation=accumulation)
    try:
        if feat is not None:
            job.set_features(feat)
        scores, pairs = [job.step().cpu().numpy()], [job.weighted_pairs()]
        sums, nh, nm = job.stir()
        sums = sums.cpu().numpy()
        for _ in range(steps_after):
            scores.append(job.step().cpu().numpy())
            pairs.append(job.weighted_pairs())
        return sums, nh, nm, scores, pairs
    finally:
        job.close()


def one_shard():
    if "one_shard" not in _CACHE:
        _CACHE["one_shard"] = gpu_stir(*case("mixed")[:4])
    return _CACHE["one_shard"]


def rel_err(a, ref):
    return float(np.max(np.abs(a - ref) / np.abs(ref)))


@pytest.mark.parametrize("name", list(SHAPES))
def test_sums_match_the_model(name):
    x, y, recip, isd, m_sums, m_h, m_m, _ = case(name)
    sums, nh, nm = one_shard()[:3] if name == "mixed" else gpu_stir(x, y, recip, isd)[:3]
    assert (nh, nm) == (m_h, m_m)
    assert np.all(m_sums > 0)
    err = rel_err(sums, m_sums)
    print(f"{name}: max relative error of the four sums {err:.3e}")
    assert err <= SUM_TOL
    # a discrete feature's squares are its diffs
    assert np.array_equal(sums[1][isd], sums[0][isd]) and np.array_equal(sums[3][isd], sums[2][isd])


def test_feature_subset_of_both_kinds():
    x, y, recip, isd = case("mixed")[:4]
    feat = np.array([1, 3, 7, 19, 22, 25, 30, 38])
    sums, nh, nm = gpu_stir(x, y, recip, isd, feat=feat)[:3]
    m_sums, m_h, m_m, _ = stir_np.stir_sums(np.ascontiguousarray(x[:, feat]), y, recip[feat],
                                            isd[feat])
    assert sums.shape == (4, feat.size) and (nh, nm) == (m_h, m_m)
    err = rel_err(sums, m_sums)
    print(f"subset: max relative error {err:.3e}")
    assert err <= SUM_TOL


def test_t_statistics_match_the_model():
    from fastselect_amd import _lib
    m_sums, m_h, m_m, _ = case("mixed")[4:]
    sums, nh, nm = one_shard()[:3]
    _, _, t, df = _lib.stir_statistics(sums, nh, nm)
    _, _, m_t, m_df, _ = stir_np.statistics(m_sums, m_h, m_m)
    assert df == m_df
    tol = stir_np.t_tolerance(m_sums, m_h, m_m, SUM_TOL)
    print(f"max |t - model| / tolerance {np.max(np.abs(t - m_t) / tol):.3e}")
    assert np.all(np.abs(t - m_t) <= tol)


def test_shards_add_up(hooks):
    x, y, recip, isd = case("mixed")[:4]
    hooks("shards", 3)
    sums, nh, nm = gpu_stir(x, y, recip, isd)[:3]
    ref, rh, rm = one_shard()[:3]
    assert (nh, nm) == (rh, rm)
    np.testing.assert_allclose(sums, ref, rtol=ADD_TOL, atol=0)


def test_row_ranges_add_up():
    x, y, recip, isd = case("mixed")[:4]
    a, ah, am = gpu_stir(x, y, recip, isd, rows=(0, 150))[:3]
    b, bh, bm = gpu_stir(x, y, recip, isd, rows=(150, 300))[:3]
    ref, rh, rm = one_shard()[:3]
    assert (ah + bh, am + bm) == (rh, rm)
    assert np.all(a > 0) and np.all(b > 0)
    np.testing.assert_allclose(a + b, ref, rtol=ADD_TOL, atol=0)


def test_one_tile_per_chunk(hooks):
    x, y, recip, isd = case("mixed")[:4]
    hooks("stir_chunk", 1)
    sums = gpu_stir(x, y, recip, isd)[0]
    np.testing.assert_allclose(sums, one_shard()[0], rtol=ADD_TOL, atol=0)


def segments_case():
    """The n600-p140 sums with the stage's own split (15 tiles: one tile per
    segment, one chunk), once per session."""
    if "segments" not in _CACHE:
        _CACHE["segments"] = gpu_stir(*case("n600-p140")[:4])
    return _CACHE["segments"]


# tiles per segment, tiles per chunk (0: the default, one chunk).  The 15 tiles
# run (0,0) .. (0,4), (1,1) .. (1,4), (2,2) ..: every segment longer than one
# tile carries A rows over tiles of a row block or reloads them where the row
# block changes, and takes a tile's column 0 weights from the previous tile's
# last prefetch.  2: seven whole segments and a ragged one; 4: 4 + 4 + 4 + 3;
# 15: one segment over all five row blocks.  With chunks: 2 / 4 gives chunks
# of 4, 4, 4, 3 tiles (two segments each, the last ragged); 4 / 5 is taken up
# to 8 and gives 8 + 7 (segments 4, 4 | 4, 3: seg0 = 2 in the second chunk);
# 3 / 7 is taken up to 9 and gives 9 + 6.
@pytest.mark.parametrize("seg_len,chunk", [(2, 0), (4, 0), (15, 0), (2, 4), (4, 5), (3, 7)])
def test_multi_tile_segments(hooks, seg_len, chunk):
    x, y, recip, isd, m_sums, m_h, m_m, _ = case("n600-p140")
    ref, rh, rm = segments_case()[:3]
    hooks("stir_seg_len", seg_len)
    if chunk:
        hooks("stir_chunk", chunk)
    sums, nh, nm = gpu_stir(x, y, recip, isd)[:3]
    assert (nh, nm) == (rh, rm) == (m_h, m_m)
    err = rel_err(sums, m_sums)
    print(f"seg_len {seg_len}, chunk {chunk}: max relative error {err:.3e}")
    assert err <= SUM_TOL
    np.testing.assert_allclose(sums, ref, rtol=ADD_TOL, atol=0)


def test_segments_with_shards_and_rows(hooks):
    """Multi-tile segments on a shard's tile list (every third tile: the row
    block changes inside most segments) and on a row range."""
    x, y, recip, isd = case("n600-p140")[:4]
    ref = segments_case()[0]
    hooks("stir_seg_len", 2)
    hooks("shards", 3)
    np.testing.assert_allclose(gpu_stir(x, y, recip, isd)[0], ref, rtol=ADD_TOL, atol=0)
    hooks("shards", 0)
    a = gpu_stir(x, y, recip, isd, rows=(0, 333))[0]
    b = gpu_stir(x, y, recip, isd, rows=(333, 600))[0]
    np.testing.assert_allclose(a + b, ref, rtol=ADD_TOL, atol=0)


def test_step_is_unchanged_by_stir():
    x, y, recip, isd = case("mixed")[:4]
    _, _, _, scores, pairs = gpu_stir(x, y, recip, isd, steps_after=1)
    assert np.array_equal(scores[0], scores[1])
    assert pairs[0] == pairs[1] and pairs[0] > 0


def test_reference_accumulation():
    x, y, recip, isd, m_sums, m_h, m_m, _ = case("mixed")
    sums, nh, nm = gpu_stir(x, y, recip, isd, accumulation="reference")[:3]
    assert (nh, nm) == (m_h, m_m)
    err = rel_err(sums, m_sums)
    print(f"reference accumulation: max relative error {err:.3e}")
    assert err <= SUM_TOL


def test_estimator_ranks_the_planted_pair_as_the_cpu_backend():
    from fastselect_amd import MultiSURF
    x, y = case("mixed")[:2]
    gpu = MultiSURF(n_features_to_select=2, backend="gpu").stir_test(x, y)
    cpu = MultiSURF(n_features_to_select=2, backend="cpu").stir_test(x, y)
    assert gpu.effective_backend_ == "gpu"
    order = lambda est: np.argsort(est.stir_t_)[::-1][:2].tolist()  # noqa: E731
    assert order(gpu) == order(cpu) and set(order(gpu)) == {3, 25}
    assert gpu.stir_p_values_[3] < 1e-6 and gpu.stir_p_values_[25] < 1e-6
    assert (gpu.stir_n_hit_pairs_, gpu.stir_n_miss_pairs_) == (14474, 13046)
    assert gpu.stir_df_ == cpu.stir_df_


def test_refusals_on_the_device():
    import torch
    from fastselect_amd import _lib
    x, y, recip, isd = case("mixed")[:4]
    n, p = x.shape
    s = torch.zeros(4 * p, dtype=torch.float64, device="cuda")
    rs = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    cn = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # the plans run on streams of their own
    pl = _lib.Plan("gpu", x, y, recip, isd)
    try:
        with pytest.raises(ValueError, match="fs_plan_select"):
            pl.stir(s.data_ptr())
    finally:
        pl.close()
    torch.cuda.synchronize()
    pl = _lib.Plan("gpu", x, y, recip, isd, use_star=True)
    try:
        pl.pass1(rs.data_ptr())
        pl.select(rs.data_ptr(), cn.data_ptr())
        with pytest.raises(RuntimeError, match="MultiSURF\\*"):
            pl.stir(s.data_ptr())
    finally:
        pl.close()
