"""``MDR.rank_interactions`` on the CPU backend: ``fit``'s attributes with
``fit``'s values, and the ranked list against a numpy restatement built from
``mdr_np.lookup`` / ``predict`` (the GPU twin is in test_gpu_mdr_top.py)."""
import numpy as np
import pytest

import mdr_np
from fastselect_amd import MDR, _lib
from mdr_top_np import check_estimator


@pytest.mark.parametrize("n,p,k,cv,n_top", [(203, 40, 2, 5, 25), (203, 14, 3, 3, 7),
                                            (33, 5, 1, 2, 9)])
def test_rank_interactions_equals_fit_and_numpy(n, p, k, cv, n_top):
    est = check_estimator("cpu", n, p, k, cv, n_top)
    # the fitted model is its folds' best in best_cvc_ folds
    row = [tuple(c) for c in est.top_interactions_.tolist()]
    if tuple(est.best_interaction_) in row:
        assert est.top_cvc_[row.index(tuple(est.best_interaction_))] == est.best_cvc_
    assert np.all(est.top_cvc_ <= est.top_fold_hits_) and np.all(est.top_fold_hits_ <= cv)


def test_planted_pair_leads_the_list():
    X, y = mdr_np.planted(203, 40)
    est = MDR(k=2, cv=5, backend="cpu").rank_interactions(X, y, n_top=10)
    assert tuple(est.top_interactions_[0]) == (1, 38)
    assert est.top_cvc_[0] == 5 and est.top_fold_hits_[0] == 5
    assert np.all(np.diff(est.top_training_ba_) <= 0)


def test_n_top_is_checked():
    X, y = mdr_np.planted(50, 6)
    with pytest.raises(ValueError, match="n_top"):
        MDR(k=2, cv=2, backend="cpu").rank_interactions(X, y, n_top=0)
    with pytest.raises(ValueError, match=str(_lib.MDR_MAX_TOP)):
        MDR(k=2, cv=2, backend="cpu").rank_interactions(X, y, n_top=_lib.MDR_MAX_TOP + 1)
    # fit's own checks come through _validate
    with pytest.raises(ValueError, match="binary"):
        MDR(k=2, cv=2, backend="cpu").rank_interactions(X, np.arange(50) % 3, n_top=3)
    assert "n_top" not in MDR().get_params()
