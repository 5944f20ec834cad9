"""Discrete mutual information and mRMR on the CPU backend (fs_mi_cpu.cpp,
fastselect_amd/mRMR.py) against the numpy restatement (mi_np.py), and the
estimator behaviours of the reference's own tests, restated.

Tolerances: counts are integers and compared exactly.  A mutual information
is a sum of at most 1024 terms pxy * log(r) with 1/n <= r <= n and
sum(pxy) = 1: a few ulps per term plus a <= 1 ulp log bound the error of the
sum near 4e-12 bits for n < 2^31, so the absolute 1e-10 used here leaves
about 25x over that bound, and a wrong count (which moves MI by about 1/n or
more) cannot hide in it.

The shapes are mi_np.ALL_SHAPES: the GPU tests' own (test_gpu_mi.py lists
them), the state counts 4 to 29 of mi_np.GEOMETRY and the long sample axes of
mi_np.LONG included.
"""
import math

import numpy as np
import pytest
from sklearn.exceptions import NotFittedError

import mi_np

TOL = 1e-10


@pytest.mark.parametrize("name", sorted(mi_np.ALL_SHAPES))
def test_cpu_backend_equals_numpy(name):
    from fastselect_amd import _lib
    X, y, S, rel, red, cnt = mi_np.case(name, mi_np.ALL_SHAPES[name])
    r, R, c = _lib.mi_matrices("cpu", X, y, S, want_counts=True)
    assert np.array_equal(c, cnt)
    assert np.abs(r - rel).max() <= TOL
    assert np.abs(R - red).max() <= TOL
    # the thread count changes neither counts nor bits
    r1, R1 = _lib.mi_matrices("cpu", X, y, S, n_jobs=1)
    assert np.array_equal(r1, r) and np.array_equal(R1, R)


@pytest.mark.parametrize("states", [3, 12])   # the plane route and the table walk
def test_matrix_properties(states):
    from fastselect_amd import mutual_information as mi
    X, y = mi_np.uniform(150, 8, states, 31)
    X = X.copy()
    # a duplicated column, next to its original: a pair takes its rows from
    # the earlier column, so only neighbours meet every third column on the
    # same side of the table (and so in the same order of float64 operations)
    X[:, 3] = X[:, 2]
    X[:, 6] = 1            # a constant column (not state 0)
    rel, red = mi.calculate_mi_matrices(X, y, backend="cpu")
    assert rel.shape == (8,) and red.shape == (8, 8)
    assert np.array_equal(red, red.T)
    assert not np.diag(red).any()
    keep = [j for j in range(8) if j not in (2, 3)]
    assert np.array_equal(red[2, keep], red[3, keep])
    assert rel[2] == rel[3]
    assert rel[6] == 0.0 and not red[6].any() and not red[:, 6].any()
    # I(x; x) is the column's entropy -- up to the eps of the stated
    # expressions, which lowers it by sum_a 1e-12 / q_a / log(2): 1.3e-11 at
    # three even states, but 2.4e-10 at twelve, where the check does not apply
    _, cnt = np.unique(X[:, 2], return_counts=True)
    q = cnt / 150.0
    if states == 3:
        assert abs(red[2, 3] - float(-(q * np.log2(q)).sum())) <= TOL
    rel_n, red_n = mi.calculate_mi_matrices(X, y, backend="cpu", unit="nat")
    assert np.abs(rel_n - rel * math.log(2.0)).max() <= TOL
    assert np.abs(red_n - red * math.log(2.0)).max() <= TOL


def test_single_pair_and_validation():
    from fastselect_amd import mutual_information as mi
    X, y = mi_np.uniform(120, 3, 4, 32)
    rel, red = mi.calculate_mi_matrices(X, y, backend="cpu")
    assert mi.calculate_mi_single_pair(X[:, 0], y, backend="cpu") == rel[0]
    assert mi.calculate_mi_single_pair(X[:, 0], X[:, 2], backend="cpu") == red[0, 2]
    with pytest.raises(ValueError, match="1‑D arrays of equal length"):
        mi.calculate_mi_single_pair(X[:, 0], y[:-1], backend="cpu")
    with pytest.raises(ValueError, match="X must be 2‑D and y 1‑D"):
        mi.calculate_mi_matrices(X[:, 0], y, backend="cpu")
    with pytest.raises(ValueError, match="integer‑coded array"):
        mi.calculate_mi_matrices(X.astype(np.float64), y, backend="cpu")
    with pytest.raises(ValueError, match="negative values"):
        mi.calculate_mi_matrices(X.astype(np.int64) - 1, y, backend="cpu")
    big = X.astype(np.int64)
    big[0, 0] = 256
    with pytest.raises(ValueError, match="256"):
        mi.calculate_mi_matrices(big, y, backend="cpu")
    big[0, 0] = 255   # 256 states: the CPU backend's cap
    rel, _ = mi.calculate_mi_matrices(big, y, backend="cpu")
    want, _, _ = mi_np.matrices(big, y, 256)
    assert np.abs(rel - want).max() <= TOL


def test_more_than_32_states_on_the_gpu_backend():
    from fastselect_amd import _lib
    from fastselect_amd import mutual_information as mi
    X, y = mi_np.uniform(90, 3, 33, 33)
    X = X.copy()
    X[0, 0] = 32
    if _lib.gpu_available():
        with pytest.raises(RuntimeError, match="GPU backend supports ≤32 states"):
            mi.calculate_mi_matrices(X, y, backend="gpu")
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            mi.calculate_mi_matrices(X, y, backend="gpu")
    rel, _ = mi.calculate_mi_matrices(X, y, backend="auto")   # answers from the CPU
    assert np.abs(rel - mi_np.matrices(X, y, 33)[0]).max() <= TOL


# ---- the estimator (the reference's tests/test_mrmr.py, restated) ----------

@pytest.fixture(scope="module")
def discrete_data():
    """100 x 20 quartile-binned make_classification data with 4 classes."""
    from sklearn.datasets import make_classification
    X, y = make_classification(n_samples=100, n_features=20, n_informative=5, n_redundant=2,
                               n_classes=4, random_state=42)
    edges = np.percentile(X, [25, 50, 75], axis=0)
    Xd = np.empty_like(X, dtype=np.int64)
    for i in range(X.shape[1]):
        Xd[:, i] = np.digitize(X[:, i], bins=edges[:, i])
    return Xd, y


def test_constructor_errors():
    from fastselect_amd import _lib, mRMR
    with pytest.raises(ValueError, match="Method must be either 'MID' or 'MIQ'."):
        mRMR(n_features_to_select=5, method="INVALID_METHOD")
    with pytest.raises(ValueError, match="Backend must be either 'cpu' or 'gpu'"):
        mRMR(n_features_to_select=5, backend="tpu")
    mRMR(n_features_to_select=5, backend="auto")
    if not _lib.gpu_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            mRMR(n_features_to_select=5, backend="gpu")


@pytest.mark.parametrize("method", ["MID", "MIQ"])
def test_fit_transform_shapes_and_numpy_parity(discrete_data, method):
    from fastselect_amd import mRMR
    X, y = discrete_data
    model = mRMR(n_features_to_select=5, method=method, backend="cpu").fit(X, y)
    assert model.effective_backend_ == "cpu"
    assert model.top_features_.shape == (5,) and model.top_features_.dtype == np.int32
    assert model.relevance_scores_.shape == (20,)
    assert model.redundancy_matrix_.shape == (20, 20)
    assert model.feature_importances_ is model.relevance_scores_
    assert model.n_features_in_ == 20
    assert np.array_equal(model.unique_vals_, np.arange(4))
    assert model.transform(X).shape == (100, 5)
    assert np.array_equal(model.transform(X), X[:, model.top_features_])
    assert mRMR(5, method=method, backend="cpu").fit_transform(X, y).shape == (100, 5)
    rel, red, _ = mi_np.matrices(X, y, 4)
    assert np.abs(model.relevance_scores_ - rel).max() <= TOL
    assert np.abs(model.redundancy_matrix_ - red).max() <= TOL
    assert np.array_equal(model.top_features_, mi_np.greedy(rel, red, 5, method)[0])


def test_values_are_encoded_through_the_global_dictionary():
    """Arbitrary integer values (negative ones too) select as their ranks."""
    from fastselect_amd import mRMR
    X, y = mi_np.planted(203, 37, 3, 1)
    vals = np.array([-7, 40, 1000])
    a = mRMR(4, backend="cpu").fit(vals[X], vals[y])
    b = mRMR(4, backend="cpu").fit(X, y)
    assert np.array_equal(a.unique_vals_, vals)
    assert np.array_equal(a.top_features_, b.top_features_)
    assert np.array_equal(a.redundancy_matrix_, b.redundancy_matrix_)


def test_duplicate_of_a_selected_feature_loses_to_a_cleaner_one():
    from fastselect_amd import mRMR
    rng = np.random.default_rng(42)
    n, p = 200, 10
    y = rng.integers(0, 2, n)
    X = rng.integers(0, 3, size=(n, p))
    X[:, 0] = (y + (rng.random(n) < 0.10).astype(int)) % 2
    X[:, 1] = X[:, 0]
    X[:, 9] = (y + (rng.random(n) < 0.05).astype(int)) % 2
    model = mRMR(n_features_to_select=2, method="MID", backend="cpu").fit(X, y)
    assert set(model.top_features_.tolist()) == {0, 9}


def test_pipeline(discrete_data):
    from sklearn.linear_model import LogisticRegression
    from sklearn.pipeline import Pipeline
    from fastselect_amd import mRMR
    X, y = discrete_data
    pipe = Pipeline([("mrmr", mRMR(n_features_to_select=3, backend="cpu")),
                     ("clf", LogisticRegression(random_state=42))])
    assert pipe.fit(X, y).predict(X).shape == (100,)


def test_input_validation(discrete_data):
    from fastselect_amd import mRMR
    X, y = discrete_data
    model = mRMR(n_features_to_select=5, backend="cpu")
    with pytest.raises(NotFittedError):
        model.transform(X)
    with pytest.raises(ValueError, match="n_features_to_select must be a positive integer"):
        mRMR(n_features_to_select=21, backend="cpu").fit(X, y)
    with pytest.raises(ValueError, match="n_features_to_select must be a positive integer"):
        mRMR(n_features_to_select=0, backend="cpu").fit(X, y)
    model.fit(X, y)
    with pytest.raises(ValueError,
                       match="X has 19 features, but mRMR is expecting 20 features as input."):
        model.transform(np.delete(X, 0, axis=1))
    with pytest.raises(ValueError, match="integer‑coded array"):
        mRMR(n_features_to_select=5, backend="cpu").fit(X.astype(np.float64), y)


def test_negative_codes_are_rejected_by_the_mi_functions(discrete_data):
    from fastselect_amd import mutual_information as mi
    X, y = discrete_data
    with pytest.raises(ValueError, match="negative values"):
        mi.calculate_mi_matrices(X - 2, y, backend="cpu")
    with pytest.raises(ValueError, match="negative values"):
        mi.calculate_mi_single_pair(X[:, 0], y - 1, backend="cpu")


def test_public_names():
    import fastselect_amd
    from fastselect_amd import mRMR
    assert "mRMR" in fastselect_amd.__all__
    assert mRMR.__module__ == "fastselect_amd"
    assert hasattr(fastselect_amd.mutual_information, "calculate_mi_matrices")
