"""The longdouble shrinkage model (tests/shrinkage_model.py) against sklearn's estimators and
on the edge cases the kernel has to reproduce.  CPU only."""
import numpy as np
import pytest

from porqua_amd.synthetic import factor_panel
from tests import shrinkage_model as sm

SHAPES = [(252, 1000), (60, 24), (7, 5), (33, 130), (65, 191)]


@pytest.fixture(scope="module")
def panel():
    return factor_panel(600, 1000)[1]


def _window(panel, T, n):
    return panel[100:100 + T, :n]


def test_gram_is_the_longdouble_product(panel):
    """The model's exact-piece Gram against numpy's own longdouble matmul, on a centred window
    and on one with a large mean (entries of very different magnitude)."""
    X = np.asarray(_window(panel, 33, 130), dtype=sm.LD)
    for Y in (X - X.mean(axis=0), X + 7.0, X * np.logspace(-6, 3, 130).astype(sm.LD)):
        ref = Y @ Y.T
        assert np.abs(sm.gram(Y) - ref).max() <= 1e-17 * np.abs(ref).max()


@pytest.mark.parametrize("T,n", SHAPES)
def test_model_matches_sklearn(panel, T, n):
    skc = pytest.importorskip("sklearn.covariance")
    X = _window(panel, T, n)
    lw = float(sm.stats(X, "ledoit_wolf")[3])
    oas = float(sm.stats(X, "oas")[3])
    assert abs(lw - skc.ledoit_wolf_shrinkage(X)) <= 1e-12
    assert abs(oas - skc.oas(X)[1]) <= 1e-12
    # sklearn shrinks the ddof = 0 covariance; the same intensity on the project's ddof = 1 S
    S0 = np.asarray(sm.shrunk_cov(X, "ledoit_wolf")[0], dtype=np.float64) * (T - 1) / T
    ref = skc.ledoit_wolf(X)[0]
    assert np.abs(S0 - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("T,n", SHAPES)
def test_band_restatement_matches_model(panel, T, n):
    """The float64 restatement of the kernel's algorithm stays within the moment tolerance of
    the model on the panel windows (the kernel's GPU tests ask the same of the kernel)."""
    X = _window(panel, T, n)
    for kind in sm.KINDS:
        for centred in (True, False):
            m = sm.stats(X, kind, centred)
            r = sm.band_stats_f64(X, kind, centred)
            for k in range(3):
                assert abs(r[k] - m[k]) <= 1e-12 * abs(m[k])
            assert abs(r[3] - m[3]) <= 1e-12


def test_edge_cases(panel):
    # T = 2: the centred rows are +-d, K = |d|^2/... [[1, -1], [-1, 1]]: g = f / 2, delta_LW = 0
    a, f, g, d = sm.stats(_window(panel, 2, 64), "ledoit_wolf")
    assert d == 0 and abs(g - f / 2) <= 1e-15 * f
    # a constant window: K = 0, both denominators are 0
    C = np.full((9, 6), 0.25)
    assert sm.stats(C, "ledoit_wolf")[3] == 0 and sm.stats(C, "oas")[3] == 1
    assert sm.band_stats_f64(C, "ledoit_wolf")[3] == 0 and sm.band_stats_f64(C, "oas")[3] == 1
    # one row: a = f = g = 0
    assert sm.stats(C[:1], "ledoit_wolf") == (0, 0, 0, 0) and sm.stats(C[:1], "oas") == (0, 0, 0, 1)
    # (7, 5): OAS is the clipped value, Ledoit-Wolf is interior
    X = _window(panel, 7, 5)
    a, f, g, d = sm.stats(X, "oas")
    assert d == 1 and (f + a * a) / (8 * (f - a * a / 5)) > 1
    assert abs(float(sm.stats(X, "ledoit_wolf")[3]) - 0.623) < 5e-3
    # the intensity is far from a constant across shapes
    assert 0.05 < float(sm.stats(_window(panel, 252, 1000))[3]) < 0.1
    assert 0.2 < float(sm.stats(_window(panel, 60, 24))[3]) < 0.4


def test_shrunk_cov_is_the_convex_combination(panel):
    X = _window(panel, 33, 130)
    for kind in sm.KINDS:
        S, d = sm.shrunk_cov(X, kind)
        S1 = np.cov(X, rowvar=False)
        ref = (1 - float(d)) * S1 + float(d) * np.trace(S1) / 130 * np.eye(130)
        assert np.abs(np.asarray(S, dtype=np.float64) - ref).max() <= 1e-12 * np.abs(ref).max()
        assert 0 < d < 1
