"""pq_hrp_linkage_batched, engine.hrp_weights(method=...) and HierarchicalRiskParity(linkage=...)
for the complete, average, weighted and Ward trees against the extended-precision model of
tests/hrp_linkage_model.py.

The batches are those of tests/test_hrp_gpu.py (its Case: the five-date row table, S = X_c'X_c from
torch in a buffer whose padding is NaN).  The work slabs have a pitch wider than n and are
pre-filled with a sentinel, as is a guard slab after the last date: a write past column n or past
the batch shows.  A date with Sigma = c I (the one-row window with the ridge) is compared against
the float64 model: every distance is exactly sqrt(1 / 2) there and the rounding of the updates
decides the ties (tests/test_hrp_linkage_model.py checks that no other date needs this).
"""
import functools
import math

import numpy as np
import pandas as pd
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.backtest import Backtest
from porqua_amd.covariance import Covariance
from porqua_amd.optimization import HierarchicalRiskParity
from tests import hrp_linkage_model as lm
from tests import hrp_model as m
from tests import test_hrp_gpu as g

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
U = 2.0 ** -53
PAD, SCALE = g.PAD, g.SCALE
OK, BAD = _lib.PQ_HRP_OK, _lib.PQ_HRP_BAD_INPUT
CODE = _lib.HRP_METHODS
# Per method (X_TOL, D_TOL, VAR_TOL): ten times the largest relative deviation of the float64 numpy
# restatement of the kernel (hrp_linkage_model.hrp_f64) from the longdouble model over every case,
# ridge and well-posed date below and the two n = 1024 windows, measured on the CPU
# (tests/test_hrp_linkage_model.py keeps them honest).  The worst cases:
#   x          complete 2.80e-12, average 2.80e-12, weighted 3.12e-13, ward 3.12e-13, each at n = 130,
#              T = 7 on the half window (three rows: Sigma has rank two, the cluster variances cancel);
#   distance   2.08e-8 for all four at n = 257, T = 252 on the short window (three rows, two assets
#              7e-5 apart: the distance is the root of 1 - rho), the leaf merge that sets single's too;
#   x' Sigma x complete 3.40e-14 (n = 130, T = 7, short), average 2.52e-14 (n = 130, T = 7, half),
#              weighted 1.15e-14 (n = 64, T = 7, short), ward 3.37e-15 (n = 257, T = 252, short).
TOL = {"complete": (2.8e-11, 2.1e-7, 3.4e-13), "average": (2.8e-11, 2.1e-7, 2.5e-13),
       "weighted": (3.1e-12, 2.1e-7, 1.2e-13), "ward": (3.1e-12, 2.1e-7, 3.4e-14)}


def _launch(S, n, alpha, c, method, scale=SCALE, link=True, work=True, ldw=None, entry=True):
    """pq_hrp_linkage_batched on the device batch S (B, ld, ld).  Outputs are pre-filled with -7;
    the work slabs (pitch n + PAD, one guard slab more than dates) with -9.  Returns (rc, x, order,
    Z, stats, status) as numpy."""
    lib = _lib.load()
    dev = S.device
    B = int(S.shape[0])
    a_d = torch.as_tensor(np.asarray(alpha, dtype=np.float64), device=dev)
    c_d = torch.as_tensor(np.asarray(c, dtype=np.float64), device=dev)
    x = torch.full((B, n + 1), -7.0, dtype=F64, device=dev)
    order = torch.full((B, n + 2), -7, dtype=torch.int32, device=dev)
    Zc = torch.full((B * max(n - 1, 0) * 4 + 1,), -7.0, dtype=F64, device=dev)
    stats = torch.full((B, 2), -7.0, dtype=F64, device=dev)
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    pitch = n + PAD
    W = torch.full((B + 1, n, pitch), -9.0, dtype=F64, device=dev)
    code = CODE[method] if isinstance(method, str) else method
    rc = lib.pq_hrp_linkage_batched(S.data_ptr(), int(S.shape[1]), n, B, a_d.data_ptr(), c_d.data_ptr(), float(scale),
                                    code, W.data_ptr() if work else None, pitch if ldw is None else ldw,
                                    x.data_ptr(), n + 1, order.data_ptr(), n + 2, Zc.data_ptr() if link else None,
                                    stats.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    xh, oh, zh, Wh = x.cpu().numpy(), order.cpu().numpy(), Zc.cpu().numpy(), W.cpu().numpy()
    assert np.all(Wh[:, :, n:] == -9.0) and np.all(Wh[B] == -9.0)          # past column n, past the batch
    assert rc == 0 or np.all(Wh == -9.0)
    assert rc != 0 or (np.all(xh[:, n] == -7.0) and np.all(oh[:, n:] == -7) and zh[-1] == -7.0)
    return rc, xh[:, :n], oh[:, :n], zh[:-1].reshape(B, max(n - 1, 0), 4), stats.cpu().numpy(), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(n, T, d, c, method):
    """The reference of date d of the case: the longdouble model, or the float64 one where
    Sigma = c I; None: bad input.  Computed once and shared."""
    case = g._case(n, T)
    Sig = m.sigma(case.Sh[d], case.alpha[d], c)
    if Sig is None:
        return None
    if n > 1 and lm.is_scaled_identity(case.Sh[d]):
        return lm.hrp_f64(case.Sh[d], case.alpha[d], c, method, SCALE) + (Sig,)
    return lm.hrp(Sig, method, SCALE) + (Sig,)


def _assert_date(out, d, ref, n, method, what=""):
    """Date d of a launch against a model's (x, order, Z, stats, Sigma)."""
    _, x, order, Z, stats, status = out
    xm, om, Zm, sm_, Sig = ref
    x_tol, d_tol, var_tol = TOL[method]
    assert status[d] == OK, (what, d)
    assert np.array_equal(order[d], om), (what, d)
    assert np.array_equal(Z[d][:, [0, 1, 3]], np.asarray(Zm[:, [0, 1, 3]], dtype=np.float64)), (what, d)
    ex = float(np.max(np.abs(x[d] - xm) / xm))
    dm = np.asarray(Zm[:, 2])
    ed = float(np.max(np.abs(Z[d][:, 2] - dm) / np.where(dm > 0, dm, 1))) if n > 1 else 0.0
    ev = abs(stats[d, 0] - sm_[0]) / sm_[0]
    ssum = abs(float(np.sum(x[d].astype(LD)) - LD(SCALE)))
    print(f"{what} {method} date={d}: x {ex:.2e} dist {ed:.2e} var {ev:.2e} gap {stats[d, 1]:.3e} "
          f"(model {sm_[1]:.3e}) sum-scale {ssum:.1e}")
    assert ex <= x_tol and ed <= d_tol and ev <= var_tol, (what, d, ex, ed, ev)
    # a leaf's weight is a product of at most ceil(log2 n) splits, each pair summing to one within an ulp
    assert ssum <= 4 * U * (math.ceil(math.log2(max(n, 2))) + 1) * SCALE, (what, d, ssum)
    assert np.all(x[d] > 0)
    if n <= 2:
        assert stats[d, 1] == np.inf
    else:   # a difference of two distances, each within d_tol of the model's
        assert abs(stats[d, 1] - sm_[1]) <= 2 * d_tol * float(dm.max()), (what, d)


@pytest.mark.parametrize("method", lm.METHODS)
@pytest.mark.parametrize("ridge", [False, True])
@pytest.mark.parametrize("T", m.TS)
@pytest.mark.parametrize("n", m.NS)
def test_kernel_matches_model(device, n, T, ridge, method):
    """order and the link's children and sizes equal the model's; distances, x and stats within the
    measured tolerances; sum(x) = scale; the single-row date without a ridge (Sigma = 0) is bad
    input and leaves its neighbours alone; nothing is written past column n of a work row or past
    the last date's slab (_launch)."""
    case = g._case(n, T)
    c = m.RIDGE if ridge else 0.0
    out = _launch(case.S, n, case.alpha, np.full(5, c), method)
    assert out[0] == 0
    if not ridge:
        assert _ref(n, T, 4, c, method) is None
    for d in range(5):
        ref = _ref(n, T, d, c, method)
        if ref is None:
            g._assert_bad(out, d)
        else:
            _assert_date(out, d, ref, n, method, f"n={n} T={T} c={c:g}")
    if n == 1:
        assert np.all(out[1][out[5] == OK] == SCALE) and np.all(out[2][out[5] == OK] == 0)


@functools.lru_cache(maxsize=None)
def _big():
    """The n = PQ_HRP_NMAX window: S on the device (pitch n + 4: the 16-byte row loads, every
    thread with four live columns) and on the host."""
    n = lm.N_BIG
    dev = engine.default_device()
    X = torch.from_numpy(g._panel(n)).to(dev)[torch.from_numpy(lm.big_rows().astype(np.int64)).to(dev)]
    Xc = X - X.mean(dim=0)
    S = torch.full((1, n + 4, n + 4), float("nan"), dtype=F64, device=dev)
    S[0, :n, :n] = Xc.T @ Xc
    return S, S[0, :n, :n].cpu().numpy()


@pytest.mark.parametrize("method", lm.METHODS)
@pytest.mark.parametrize("ridge", [False, True])
def test_largest_n_matches_model(device, ridge, method):
    """n = PQ_HRP_NMAX: the largest LDS footprint, every thread owning four live columns."""
    assert lm.N_BIG == _lib.PQ_HRP_NMAX
    n, al, c = lm.N_BIG, 1.0 / (lm.T_BIG - 1), m.RIDGE if ridge else 0.0
    S, Sh = _big()
    out = _launch(S, n, [al], [c], method)
    assert out[0] == 0
    Sig = m.sigma(Sh, al, c)
    _assert_date(out, 0, lm.hrp(Sig, method, SCALE) + (Sig,), n, method, f"n={n} c={c:g}")


def _scipy(D, method):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    Z = hier.linkage(squareform(D, checks=False), method)
    return Z, hier.leaves_list(Z)


@pytest.mark.parametrize("method", lm.METHODS)
def test_all_ties_and_scaled_identity_give_scipys_tree(device, method):
    """The 8 x 8 all-ties matrix and Sigma = c I at n = 16, 65 and 257: children, sizes and leaf
    order are SciPy's, distances within 8 ulp, the weights scale / n."""
    from tests.test_hrp_model import all_ties
    dev = engine.default_device()
    for n, Sig, al, c in [(8, all_ties(), 1.0, 0.0)] + [(n, np.zeros((n, n)), 1.0, m.RIDGE) for n in (16, 65, 257)]:
        S = torch.full((1, n + PAD, n + PAD), float("nan"), dtype=F64, device=dev)
        S[0, :n, :n] = torch.from_numpy(Sig)
        out = _launch(S, n, [al], [c], method)
        assert out[0] == 0 and out[5][0] == OK
        Zs, leaves = _scipy(lm.kernel_distance(Sig, al, c), method)
        assert np.array_equal(out[3][0][:, [0, 1, 3]], Zs[:, [0, 1, 3]]), n
        assert np.array_equal(out[2][0], leaves), n
        assert np.abs(out[3][0][:, 2] / Zs[:, 2] - 1).max() <= 8 * U, n
        assert np.abs(out[1][0] * n / SCALE - 1).max() <= 8 * U, n


@pytest.mark.parametrize("n", [17, 130])
def test_single_through_the_new_entry_point_is_pq_hrp_batched(device, n):
    case = g._case(n, 63)
    c = np.full(5, m.RIDGE)
    old = g._launch(case.S, n, case.alpha, c)
    new = _launch(case.S, n, case.alpha, c, "single", work=False)
    assert old[0] == 0 and new[0] == 0
    for p, q in zip(old[1:], new[1:]):
        assert np.array_equal(p, q, equal_nan=True)


def _neighbours_unchanged(full, clean, bad_dates):
    keep = [d for d in range(5) if d not in bad_dates]
    for p, q in zip(full[1:], clean[1:]):
        assert np.array_equal(p[keep], q[keep], equal_nan=True)


def test_non_finite_entries_and_coefficients_are_bad_input_and_isolated(device):
    """A NaN in column n - 1 of every row in turn (not mirrored: only the check of its own entry
    can show it, in the lower triangle too), and a negative or non-finite alpha or c."""
    n, method = 17, "average"
    case = g._case(n, 63)
    c = np.full(5, m.RIDGE)
    clean = _launch(case.S, n, case.alpha, c, method)
    assert clean[0] == 0 and np.all(clean[5] == OK)
    for r, col in [(r, n - 1) for r in range(n - 1)] + [(n - 1, 0), (n - 1, n - 2)]:
        S = case.S.clone()
        S[3, r, col] = float("nan")
        out = _launch(S, n, case.alpha, c, method)
        assert out[0] == 0
        g._assert_bad(out, 3)
        _neighbours_unchanged(out, clean, [3])
    for which, value in (("a", -1.0), ("a", float("nan")), ("a", float("inf")), ("c", -1e-9), ("c", float("nan")),
                         ("c", float("inf"))):
        al, cc = case.alpha.copy(), c.copy()
        (al if which == "a" else cc)[2] = value
        out = _launch(case.S, n, al, cc, method)
        assert out[0] == 0
        g._assert_bad(out, 2)
        _neighbours_unchanged(out, clean, [2])


@pytest.mark.parametrize("method", lm.METHODS)
def test_identical_launches_are_bitwise_equal_and_link_is_optional(device, method):
    case = g._case(257, 63)
    c = np.full(5, m.RIDGE)
    one, two = _launch(case.S, 257, case.alpha, c, method), _launch(case.S, 257, case.alpha, c, method)
    for p, q in zip(one[1:], two[1:]):
        assert np.array_equal(p, q, equal_nan=True)
    nolink = _launch(case.S, 257, case.alpha, c, method, link=False)
    assert nolink[0] == 0 and np.all(nolink[3] == -7.0)
    for i in (1, 2, 4, 5):
        assert np.array_equal(one[i], nolink[i], equal_nan=True)


@pytest.mark.parametrize("kw", [{"method": -1}, {"method": 5}, {"method": "ward", "work": False},
                                {"method": "complete", "ldw": 16}])
def test_host_argument_checks(device, kw):
    case = g._case(17, 63)
    rc, x, order, Z, stats, status = _launch(case.S, 17, case.alpha, np.zeros(5), **kw)
    assert rc != 0 and _lib.load().pq_last_error()
    assert np.all(x == -7.0) and np.all(order == -7) and np.all(Z == -7.0) and np.all(stats == -7.0)
    assert np.all(status == -7)   # nothing launched


# ---- engine / API -----------------------------------------------------------------------------

def _same(p, q):
    return torch.equal(torch.nan_to_num(p.to(F64), nan=-3.0), torch.nan_to_num(q.to(F64), nan=-3.0))


@pytest.mark.parametrize("method", lm.METHODS)
def test_engine_chunks_and_model(device, method):
    """hrp_weights(method=...) on the row table: a two-date chunk equals the one-chunk call bitwise,
    the well-posed dates are the model's (Ward is reachable here), the empty batch works."""
    n, T = 37, 63
    pan = engine.Panel(g._panel(n))
    rows, lens = m.case_rows(n, T)
    rd, td = pan.rows_to_device(rows, lens)
    full = engine.hrp_weights(pan, rd, td, c=m.RIDGE, linkage=True, method=method)
    assert list(full[3].cpu().numpy()) == [OK, OK, OK, OK, BAD]        # one row: no sample covariance
    ld = engine.round_up(n, 64)
    two = engine.hrp_weights(pan, rd, td, c=m.RIDGE, linkage=True, method=method, chunk_bytes=2 * 8 * ld * ld)
    for p, q in zip(full, two):
        assert _same(p, q)
    Sd = pan.cov(rd, td)[:, :n, :n].cpu().numpy()
    x, order, stats, status, Z = (v.cpu().numpy() for v in full)
    for d in range(4):
        Sig = m.sigma(Sd[d], 1.0, m.RIDGE)
        got = (x[d] * (SCALE / 1.0), order[d], Z[d], stats[d])
        ref = lm.hrp(Sig, method, 1.0)
        assert lm.same_tree(ref, got), d
        assert float(np.max(np.abs(x[d] - ref[0]) / ref[0])) <= TOL[method][0], d
    xe, oe, se, ste, ze = engine.hrp_weights(pan, rd[:0], td[:0], linkage=True, method=method)
    assert xe.shape == (0, n) and oe.shape == (0, n) and se.shape == (0, 2) and ste.shape == (0,) and ze.shape == (0, n - 1, 4)


def test_engine_rejects_an_unknown_method(device):
    pan = engine.Panel(g._panel(37))
    rows, lens = m.case_rows(37, 63)
    rd, td = pan.rows_to_device(rows, lens)
    for name in ("centroid", "median", "Ward", ""):
        with pytest.raises(ValueError, match="method"):
            engine.hrp_weights(pan, rd, td, method=name)


def test_solve_matches_model_and_rejects(device):
    X = g._frame(37, 100).iloc[5:65]
    opt = HierarchicalRiskParity(linkage="average")
    ok, w = g._solve_one(opt, X, budget=SCALE)
    assert ok and opt.results["status"] is True and set(opt.results) == {"weights", "status", "order", "linkage"}
    pan = engine.Panel(X.to_numpy())
    rd, td = pan.rows_to_device(np.arange(60, dtype=np.int32)[None], np.array([60], dtype=np.int32))
    Sd = pan.cov(rd, td)[0, :37, :37].cpu().numpy()
    xm, om, Zm, _ = lm.hrp(m.sigma(Sd, 1.0, 0.0), "average", SCALE)
    assert opt.results["order"] == [X.columns[i] for i in om]
    assert np.array_equal(opt.results["linkage"][:, [0, 1, 3]], np.asarray(Zm[:, [0, 1, 3]], dtype=np.float64))
    assert float(np.max(np.abs(w - xm) / xm)) <= TOL["average"][0]
    # and it is not the single-linkage portfolio
    assert not np.array_equal(om, m.hrp(m.sigma(Sd, 1.0, 0.0), SCALE)[1])
    for name in ("centroid", "median"):
        with pytest.raises(NotImplementedError, match="linkage"):
            HierarchicalRiskParity(linkage=name)


def test_backtest_batched_equals_serial_bitwise(device):
    width, n = 60, 37
    X = g._frame(n, 160)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + 12]]
    W, last = [], []
    for batched in (True, False):
        opt = HierarchicalRiskParity(covariance=Covariance(method="pearson"), linkage="complete")
        bs = g._service(opt, X, rebdates, width, budget=SCALE)
        bs.settings["batched"] = batched
        bt = Backtest()
        bt.run(bs)
        assert [p.rebalancing_date for p in bt.strategy.portfolios] == rebdates
        if batched:
            assert bt.stats["path"] == "hrp" and bt.stats["solved"] == len(rebdates)
            assert np.all(bt.stats["status"] == OK) and bt.stats["order"].shape == (12, n)
        else:
            assert bt.stats.get("path") != "hrp"
        W.append(bt.strategy.get_weights_df().to_numpy(dtype=float))
        last.append(opt.results)
    assert W[0].shape == (12, n) and np.array_equal(W[0], W[1])
    assert last[0]["order"] == last[1]["order"] and np.array_equal(last[0]["linkage"], last[1]["linkage"])
    # and they are the model's complete-linkage portfolios of each date's sample covariance
    Xv = X.to_numpy()
    for i in (0, 11):
        e = X.index.get_loc(pd.Timestamp(rebdates[i]))
        S = np.cov(Xv[e - width + 1:e + 1].T)
        xm = lm.hrp(m.sigma(S, 1.0, 0.0), "complete", SCALE)[0]
        assert float(np.max(np.abs(W[0][i] - xm) / xm)) <= 1e-9    # (numpy's covariance, not the device's bits)
