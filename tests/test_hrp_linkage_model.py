"""The linkage model of hierarchical risk parity (tests/hrp_linkage_model.py) against SciPy's
complete, average, weighted and Ward trees, bit for bit, and closed forms; and the conditions
tests/test_hrp_linkage_gpu.py relies on: on every window it compares against the longdouble model
the float64 restatement of the kernel finds that model's tree, the only windows it compares against
the float64 model instead are those with Sigma = c I, and its tolerances are ten times what the
restatement deviates from the model on those windows."""
import functools

import numpy as np
import pytest

from porqua_amd.synthetic import factor_panel
from tests import hrp_linkage_model as lm
from tests import hrp_model as m
from tests.test_hrp_model import all_ties

LD = m.LD
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _panel(n):
    return factor_panel(1100, n)[1]


def _cases():
    """(n, T, date, S float64, alpha, c) of every well-posed date the GPU test runs."""
    for n in m.NS:
        if n == 1:
            continue
        for T in m.TS:
            rows, lens = m.case_rows(n, T)
            al = m.case_alpha(lens)
            for d in range(len(lens)):
                S = m.gram(_panel(n), rows[d, :lens[d]])
                for c in (0.0, m.RIDGE):
                    if m.sigma(S, al[d], c) is not None:
                        yield n, T, d, S, al[d], c
    S = m.gram(_panel(lm.N_BIG), lm.big_rows())
    for c in (0.0, m.RIDGE):
        yield lm.N_BIG, lm.T_BIG, 0, S, 1.0 / (lm.T_BIG - 1), c


def _scipy(D, method):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    Z = hier.linkage(squareform(D, checks=False), method)
    return Z, hier.leaves_list(Z)


@functools.lru_cache(maxsize=None)
def _sweep():
    """Every case and method once: (n, T, date, c, method, the float64 Z is SciPy's in all four
    columns and its leaves SciPy's, Sigma = c I, the longdouble tree is the restatement's, the
    restatement's deviations from the longdouble model or None)."""
    out = []
    for n, T, d, S, al, c in _cases():
        D = lm.kernel_distance(S, al, c)
        Sig = m.sigma(S, al, c)
        for method in lm.METHODS:
            got = lm.hrp_f64(S, al, c, method, 0.7)
            Zs, leaves = _scipy(D, method)
            scipys = np.array_equal(Zs, got[2]) and np.array_equal(leaves, got[1])
            if lm.is_scaled_identity(S):
                out.append((n, T, d, c, method, scipys, True, None, None))
                continue
            ref = lm.hrp(Sig, method, 0.7)
            same = lm.same_tree(ref, got)
            out.append((n, T, d, c, method, scipys, False, same, lm.deviation(ref, got) if same else None))
    return out


def test_float64_chain_is_scipys_linkage_bitwise():
    """All four columns of Z, on every well-posed date of NS x TS x {0, RIDGE} and at n = 1024."""
    recs = _sweep()
    assert len(recs) == 4 * (270 + 2)
    assert {r[0] for r in recs} == set(m.NS[1:]) | {lm.N_BIG}
    bad = [r[:5] for r in recs if not r[5]]
    assert not bad, bad


@pytest.mark.parametrize("method", lm.METHODS)
def test_all_ties_tree_is_scipys(method):
    """The chain's sizes differ from the union-find's here: SciPy reports the union-find's."""
    Sig = all_ties()
    x, order, Z, stats = lm.hrp_f64(Sig, 1.0, 0.0, method)
    Zs, leaves = _scipy(lm.kernel_distance(Sig, 1.0, 0.0), method)
    assert np.array_equal(Zs, Z) and np.array_equal(leaves, order)
    assert np.abs(x * 8 - 1).max() <= 8 * U
    # (the longdouble chain may build another tree: the rounding of the updates decides the ties;
    # the weights do not depend on it)
    xl = lm.hrp(Sig, method)[0]
    assert np.abs(np.asarray(xl, dtype=np.float64) * 8 - 1).max() <= 4 * U


@pytest.mark.parametrize("method", lm.METHODS)
@pytest.mark.parametrize("rho", [-0.99, -0.4, 0.0, 0.7, 0.999])
def test_two_assets_inverse_variance(rho, method):
    s1, s2 = 0.01, 0.035
    Sig = np.array([[s1 * s1, rho * s1 * s2], [rho * s1 * s2, s2 * s2]], dtype=LD)
    x, order, Z, _ = lm.hrp(Sig, method, 0.7)
    iv = 1 / np.diag(Sig)
    assert np.abs(x - LD(0.7) * iv / iv.sum()).max() <= 1e-18
    assert list(order) == [0, 1] and list(Z[0, [0, 1, 3]]) == [0, 1, 2]
    # (Sigma's entries are float64 products: rho is within 4 u |rho| of the argument, and
    # d' = -1 / (4 d); twice that)
    d = np.sqrt((1 - LD(rho)) / 2)
    assert abs(Z[0, 2] - d) <= 2 * U * abs(rho) / float(d) + 1e-18
    xf, of, Zf, _ = lm.hrp_f64(np.asarray(Sig, dtype=np.float64), 1.0, 0.0, method, 0.7)
    assert np.abs(xf / np.asarray(x, dtype=np.float64) - 1).max() <= 8 * U and list(of) == [0, 1]


@pytest.mark.parametrize("method", lm.METHODS)
@pytest.mark.parametrize("n", [1, 2, 3, 16, 37, 65])
def test_scaled_identity_gives_equal_weights(n, method):
    """Sigma = c I: scale / n whatever the tree, in the model and in the restatement."""
    x, order, _, _ = lm.hrp(LD(m.RIDGE) * np.eye(n, dtype=LD), method, 0.7)
    assert np.abs(x * n / LD(0.7) - 1).max() <= 1e-17 and sorted(order) == list(range(n))
    xf, of, _, _ = lm.hrp_f64(np.zeros((n, n)), 1.0, m.RIDGE, method, 0.7)
    assert np.abs(xf * n / 0.7 - 1).max() <= 8 * U and sorted(of) == list(range(n))


def test_gpu_windows_have_the_models_tree_and_the_tolerances_are_sized():
    """What tests/test_hrp_linkage_gpu.py assumes.  On every window but those with Sigma = c I the
    longdouble tree (children, sizes, leaf order) is the restatement's, so float64 has to find
    it -- at n = 1024 too, where GAP_MIN cannot hold (the smallest pairwise gap is about 2e-13) and
    this condition replaces it.  The windows with Sigma = c I are the one-row windows with the
    ridge and nothing else.  Per method X_TOL, D_TOL and VAR_TOL there are ten times the largest
    relative deviation of the restatement from the model (the figures are in that file's header)."""
    from tests import test_hrp_linkage_gpu as g
    recs = _sweep()
    for n, T, d, c, method, _, identity, same, dev in recs:
        assert identity == (n != lm.N_BIG and d == 4 and c > 0), (n, T, d, c)
        assert identity or same, (n, T, d, c, method)
    for method in lm.METHODS:
        worst = np.max([r[8] for r in recs if r[4] == method and r[8] is not None], axis=0)
        print(method, "largest deviations (x, distance, variance)", worst)
        # (another BLAS may sum the restatement's products in another order: the recorded figures
        # have to hold within a factor of two, not to the digit)
        for got, tol in zip(worst, g.TOL[method]):
            assert 5 * got <= tol <= 20 * got, (method, got, tol)
