"""The hierarchical-risk-parity model (tests/hrp_model.py) against SciPy's single linkage and
closed forms, and the conditions tests/test_hrp_gpu.py relies on: the windows it runs have no two
distinct pairwise distances closer than GAP_MIN, and its tolerances are ten times what the
float64 restatement of the kernel deviates from the model on those windows."""
import functools

import numpy as np
import pytest

from porqua_amd.synthetic import factor_panel
from tests import hrp_model as m

LD = m.LD
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _panel(n):
    return factor_panel(1100, n)[1]


def _dates(n, T):
    """(date, S float64, alpha, c, Sigma longdouble) of every well-posed date of the case."""
    rows, lens = m.case_rows(n, T)
    al = m.case_alpha(lens)
    for d in range(len(lens)):
        S = m.gram(_panel(n), rows[d, :lens[d]])
        for c in (0.0, m.RIDGE):
            Sig = m.sigma(S, al[d], c)
            if Sig is not None:
                yield d, S, al[d], c, Sig


def _scipy_tree(Sig):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    D = np.asarray(m.distance(Sig), dtype=np.float64)
    Z = hier.linkage(squareform(D, checks=False), "single")
    return Z, hier.leaves_list(Z)


def all_ties(n=8, vol=0.02, rho=0.3):
    return vol * vol * ((1 - rho) * np.eye(n) + rho * np.ones((n, n)))


@pytest.mark.parametrize("n", [n for n in m.NS if n > 1])
def test_tree_is_scipys_single_linkage(n):
    for T in m.TS:
        for d, S, al, c, Sig in _dates(n, T):
            _, order, Z, _ = m.hrp(Sig)
            Zs, leaves = _scipy_tree(Sig)
            assert np.array_equal(Zs[:, [0, 1, 3]], np.asarray(Z[:, [0, 1, 3]], dtype=np.float64)), (T, d, c)
            assert np.array_equal(leaves, order), (T, d, c)
            assert np.abs(Zs[:, 2] - np.asarray(Z[:, 2], dtype=np.float64)).max() <= 4 * U


def test_all_ties_tree_is_scipys():
    Sig = all_ties()
    x, order, Z, stats = m.hrp(Sig)
    Zs, leaves = _scipy_tree(Sig)
    assert np.array_equal(Zs[:, [0, 1, 3]], np.asarray(Z[:, [0, 1, 3]], dtype=np.float64))
    assert np.array_equal(leaves, order) and stats[1] == 0.0
    assert np.abs(np.asarray(x, dtype=np.float64) - 1 / 8).max() <= 4 * U
    xf, of, Zf, _ = m.hrp_f64(Sig, 1.0, 0.0)
    assert np.array_equal(of, order) and np.array_equal(Zf[:, [0, 1, 3]], Zs[:, [0, 1, 3]])


@pytest.mark.parametrize("rho", [-0.99, -0.4, 0.0, 0.7, 0.999])
def test_two_assets_inverse_variance(rho):
    s1, s2 = 0.01, 0.035
    Sig = np.array([[s1 * s1, rho * s1 * s2], [rho * s1 * s2, s2 * s2]], dtype=LD)
    x, order, Z, _ = m.hrp(Sig, 0.7)
    iv = 1 / np.diag(Sig)
    assert np.abs(x - LD(0.7) * iv / iv.sum()).max() <= 1e-18
    assert list(order) == [0, 1] and list(Z[0, [0, 1, 3]]) == [0, 1, 2]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 37])
def test_diagonal_and_identity(n):
    rng = np.random.default_rng(n)
    d = rng.uniform(1e-4, 9e-4, n).astype(LD)
    x, _, _, _ = m.hrp(np.diag(d), 1.0)
    assert np.abs(x / ((1 / d) / (1 / d).sum()) - 1).max() <= 1e-17
    x, _, _, _ = m.hrp(np.eye(n, dtype=LD), 1.0)
    assert np.abs(x * n - 1).max() <= 1e-17
    xf, _, _, _ = m.hrp_f64(np.diag(np.asarray(d, dtype=np.float64)), 1.0, 0.0)
    assert np.abs(xf / np.asarray((1 / d) / (1 / d).sum(), dtype=np.float64) - 1).max() <= 16 * U


def test_weights_sum_to_scale():
    for n, T in ((37, 63), (130, 7), (257, 252)):
        for d, S, al, c, Sig in _dates(n, T):
            x, _, _, _ = m.hrp(Sig, 0.7)
            assert abs(x.sum() - LD(0.7)) <= 1e-17 and np.all(x > 0)


def test_gpu_windows_are_well_separated_and_sized():
    """What tests/test_hrp_gpu.py assumes: on every window it runs, two distinct pairwise distances
    of the model are at least GAP_MIN apart (about 1000 times the float64 error of a correlation),
    so float64 has to find the model's tree; and X_TOL, D_TOL and VAR_TOL there are ten times the
    largest relative deviation of the float64 restatement from the model (measured on this panel:
    8.63e-13 for x at n = 130 on a three-row window, 2.08e-8 for a link distance at n = 257 on a
    three-row window, where two assets are 7e-5 apart, 1.15e-14 for x' Sigma x)."""
    from tests import test_hrp_gpu as g
    worst = np.zeros(3)
    gap = np.inf
    for n in m.NS:
        for T in m.TS:
            for d, S, al, c, Sig in _dates(n, T):
                if n > 1:
                    gap = min(gap, m.pairwise_gap(Sig))
                dev = m.deviation(S, al, c, 0.7)
                assert dev is not None, (n, T, d, c)
                worst = np.maximum(worst, dev)
    print("smallest pairwise gap", gap, "largest deviations (x, distance, variance)", worst)
    assert gap >= m.GAP_MIN
    # (another BLAS may sum the restatement's products in another order: the recorded figures
    # have to hold within a factor of two, not to the digit)
    for got, tol in zip(worst, (g.X_TOL, g.D_TOL, g.VAR_TOL)):
        assert 5 * got <= tol <= 20 * got
