"""The NumPy model of the rank covariances (tests/rank_model.py) against SciPy's spearmanr and
kendalltau (tau-b) on small tied windows, its symmetry, unit diagonal and positive
semi-definiteness, Kendall's positive definiteness where there are more assets than rows, and the
bad-input cases (no device)."""
import numpy as np
import pytest

from tests import rank_model as rm

# |rho|, |tau| <= 1, and each side takes at most three roundings (a product, a square root, a division)
SCIPY_TOL = 4 * 2.0 ** -52
PSD_TOL = 1e-12


def _window(T, n, seed=3):
    """Normal returns with ties made on purpose: every third column rounded to one decimal of its
    scale, small values of every fourth column set to exactly zero, one -0.0 beside a +0.0."""
    X = np.random.default_rng(seed + 17 * T + n).normal(3e-4, 0.02, size=(T, n))
    X[:, ::3] = np.round(X[:, ::3], 2)
    Z = X[:, 1::4]
    Z[np.abs(Z) < 0.01] = 0.0
    if T >= 4 and n >= 2:
        X[1, 1], X[2, 1] = 0.0, -0.0
    return X


@pytest.mark.parametrize("T,n", [(2, 3), (5, 4), (17, 8), (40, 6)])
def test_model_matches_scipy(T, n):
    stats = pytest.importorskip("scipy.stats")
    X = _window(T, n)
    if T == 2:
        X[:, 0] = [0.01, -0.02]          # no constant column in the two-row window
        X[:, 1] = [0.0, 0.03]
        X[:, 2] = [-0.01, 0.02]
    worst = dict(spearman=0.0, kendall=0.0)
    sp, kd = rm.rank_cov(X, "spearman"), rm.rank_cov(X, "kendall")
    assert sp.status == rm.OK and kd.status == rm.OK
    d, _ = rm.doubled_ranks(X)
    assert np.array_equal(d, 2 * np.apply_along_axis(stats.rankdata, 0, X))   # method='average'
    assert np.array_equal(d.sum(axis=0), np.full(n, T * (T + 1)))
    assert np.array_equal(rm.kendall_diag_from_ties(X), kd.diag)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            worst["spearman"] = max(worst["spearman"], abs(sp.corr[i, j] - stats.spearmanr(X[:, i], X[:, j]).statistic))
            worst["kendall"] = max(worst["kendall"],
                                   abs(kd.corr[i, j] - stats.kendalltau(X[:, i], X[:, j], variant="b").statistic))
    print(f"model against scipy (T, n) = {(T, n)}: spearman {worst['spearman']:.2e}, kendall {worst['kendall']:.2e}")
    assert worst["spearman"] <= SCIPY_TOL and worst["kendall"] <= SCIPY_TOL


@pytest.mark.parametrize("T,n", [(5, 4), (17, 8), (30, 40), (100, 60)])
@pytest.mark.parametrize("kind", rm.KINDS)
def test_model_is_a_correlation_matrix(T, n, kind):
    X = _window(T, n)
    mod = rm.rank_cov(X, kind)
    assert mod.status == rm.OK
    assert np.array_equal(mod.corr, mod.corr.T) and np.array_equal(mod.Sigma, mod.Sigma.T)
    assert np.array_equal(np.diag(mod.corr), np.ones(n))
    assert np.array_equal(mod.counts, np.round(mod.counts)) and np.array_equal(mod.counts, mod.counts.T)
    assert np.linalg.eigvalsh(mod.corr).min() >= -PSD_TOL
    assert np.allclose(np.diag(mod.Sigma), X.var(axis=0, ddof=1), rtol=1e-13, atol=0.0)


def test_kendall_is_positive_definite_where_spearman_is_singular():
    T, n = 30, 40
    X = _window(T, n)
    rho, tau = rm.rank_cov(X, "spearman"), rm.rank_cov(X, "kendall")
    lam_rho, lam_tau = np.linalg.eigvalsh(rho.corr).min(), np.linalg.eigvalsh(tau.corr).min()
    print(f"n = {n} > T = {T}: smallest eigenvalue of rho {lam_rho:.2e}, of tau {lam_tau:.2e}")
    assert abs(lam_rho) <= PSD_TOL          # rank <= T - 1 < n
    assert lam_tau >= 1e-3
    np.linalg.cholesky(tau.Sigma)


def test_model_bad_input():
    X = _window(17, 8)
    const = X.copy()
    const[:, 2] = 0.25
    zeros = X.copy()
    zeros[:, 2] = 0.0
    zeros[::2, 2] = -0.0                    # -0.0 ties with +0.0: a constant column
    nan = X.copy()
    nan[4, 1] = np.nan
    inf = X.copy()
    inf[4, 1] = -np.inf
    for kind in rm.KINDS:
        for bad in (X[:1], const, zeros, nan, inf):
            mod = rm.rank_cov(bad, kind)
            assert mod.status == rm.BAD_INPUT and np.isnan(mod.Sigma).all() and np.isnan(mod.corr).all()
        assert rm.rank_cov(X, kind).status == rm.OK
    with pytest.raises(ValueError):
        rm.rank_cov(X, "pearson")
