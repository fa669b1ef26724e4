"""The NumPy model of the PCA factor covariance (tests/pca_cov_model.py) against independent CPU
routes on synthetic.factor_panel: the n x n eigh route, sklearn's PCA.get_covariance() (n < T
only: for n > T sklearn averages the discarded eigenvalues over T - k instead of n - k), the
trace, positive definiteness and the Marchenko-Pastur factor count at config 3's shape.

Tolerance: 1e-13 of the largest variance (observed: 8e-15 against eigh, 3e-15 against sklearn)."""
import numpy as np
import pytest

from porqua_amd.synthetic import factor_panel
from tests import pca_cov_model as pm

TOL = 1e-13
SHAPES = [(252, 1000, 12), (60, 24, 3), (40, 130, 5)]


def _window(T, n):
    """(252, 1000): the first window of config 3's panel (factor_panel(251 + 4749, 1000)), where
    l_13 / l_12 = 0.997; the small shapes: a panel of their own."""
    return factor_panel(5000, n)[1][:T] if (T, n) == (252, 1000) else factor_panel(T, n)[1]


@pytest.mark.parametrize("T,n,k", SHAPES)
def test_model_equals_the_eigh_route_keeps_the_trace_and_is_pd(T, n, k):
    X = _window(T, n)
    mod = pm.pca_cov(X, k)
    assert mod.status == pm.OK and mod.k == k and mod.Z.shape == (k, n)
    ref, sigma2 = pm.pca_cov_eigh(X, k)
    top = np.diag(ref).max()
    err = np.abs(mod.Sigma - ref).max() / top
    print(f"(T, n, k) = {(T, n, k)}: Gram route vs eigh route {err:.2e} of the largest variance")
    assert err <= TOL
    assert abs(mod.sigma2 - sigma2) <= TOL * top
    S = np.cov(X, rowvar=False)
    assert abs(np.trace(mod.Sigma) - np.trace(S)) <= TOL * np.trace(S)
    assert np.linalg.eigvalsh(mod.Sigma).min() > 0
    np.linalg.cholesky(mod.Sigma)


def test_model_equals_sklearn_where_n_is_below_T():
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    T, n, k = 60, 24, 3
    X = _window(T, n)
    mod = pm.pca_cov(X, k)
    ref = PCA(k, svd_solver="full").fit(X).get_covariance()
    err = np.abs(mod.Sigma - ref).max() / np.diag(ref).max()
    print(f"model vs sklearn at {(T, n, k)}: {err:.2e} of the largest variance")
    assert err <= TOL


def test_mp_rule_finds_the_market_and_ten_sector_factors():
    X = _window(252, 1000)
    mod = pm.pca_cov(X, "mp")
    assert mod.status == pm.OK and mod.k == 11
    assert mod.margin > 1e-6
    # the rule's k gives the Sigma of that k
    assert np.array_equal(mod.Sigma, pm.pca_cov(X, 11).Sigma)


def test_model_reports_bad_input():
    X = _window(40, 30)
    assert pm.pca_cov(X[:1], 2).status == pm.BAD_INPUT                       # a one-row window
    assert pm.pca_cov(np.full((10, 6), 0.25), 2).status == pm.BAD_INPUT      # a constant window
    low = np.outer(np.arange(8.0), np.arange(1.0, 7.0))                      # rank 1
    assert pm.pca_cov(low, 3).status == pm.BAD_INPUT
    with pytest.raises(ValueError):
        pm.pca_cov(X, 30)
