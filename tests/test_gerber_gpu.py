"""The Gerber covariance on the device: pq_gerber_cov_batched (the int8 sign panel and the
v_mfma_i32_16x16x64_i8 Gram of every date) against the NumPy model (tests/gerber_model.py), and the
public interface on top of it (engine.gerber_cov, Covariance 'gerber', MeanVariance on the dense
route, HierarchicalRiskParity, Backtest).

The counts are integers, so they and variant 1's correlation are compared bit for bit; the bars of
the floating-point results are derived below, never fitted.  Every fixture is first checked on the
host to have margin >= 1e-9 (no |x| within 1e-9 of its threshold, relatively), so that a sign cannot
depend on the last bits of the standard deviation.  The observed worst values stand beside each
bar and in profiles/gerber_pytest.txt."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import ref_pipeline as rp
from porqua_amd import _lib, engine
from porqua_amd.backtest import Backtest, BacktestService
from porqua_amd.builders import (OptimizationItemBuilder, SelectionItemBuilder, bibfn_box_constraints,
                                 bibfn_budget_constraint, bibfn_return_series, bibfn_selection_data)
from porqua_amd.constraints import Constraints
from porqua_amd.covariance import Covariance, cov_gerber
from porqua_amd.helper_functions import isPD
from porqua_amd.optimization import HierarchicalRiskParity, MeanVariance, RiskParity
from porqua_amd.optimization_data import OptimizationData
from porqua_amd.synthetic import factor_panel
from tests import gerber_model as gm
from tests import hrp_model as hm

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
OK, BAD = _lib.PQ_GERBER_OK, _lib.PQ_GERBER_BAD_INPUT
POISON = 1e150
MARGIN_MIN = 1e-9
CASES = [(2, 1), (5, 3), (17, 70), (63, 64), (64, 64), (65, 130), (100, 257), (252, 130), (300, 20), (1024, 16)]
THRESHOLDS = [0.3, 0.5, 0.9]

# variant 2's correlation: one square root (<= 1 ulp) of an exact product and one division: 4 ulp.
# A wrong count moves an entry by at least 1 / T^2 >= 9.5e-7.  Observed 0: every entry is bit for bit the model's
G2_TOL = 4 * 2.0 ** -52
# Sigma relative to sd_i sd_j: a two-pass FP64 window variance over T <= 1024 terms is within about
# (T + 4) 2^-53 = 1.2e-13, the two sd factors double that, a few roundings are added, and the bar is
# ten times that figure.  Observed 6.6e-16; the diagonal against numpy's var(ddof=1): 6.1e-16
SIGMA_TOL = 1e-12
HRP_TOL = 1e-13        # HRP weights, relative (the bar of tests/test_pca_cov_gpu.py).  Observed 1.1e-15
LINK_TOL = 1e-12       # sorted single-linkage merge distances against the model's spanning tree.  Observed 9.9e-17


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- fixtures (host) ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _panel():
    R = factor_panel(400, 257, seed=5)[1].copy()
    R[-1] = POISON
    return R


def _kernel_rows(T):
    """Three windows of up to T rows as tests/test_pca_cov_gpu.py::_kernel_case builds them --
    consecutive rows, every other row, and a shorter window whose unused slots point at the poison
    row (a valid index: a stray read shows as a wrong number, never as a fault) --, wrapped around
    the panel's 399 data rows where T needs more (a window may hold a row twice)."""
    D = _panel().shape[0]
    m = D - 1
    short = max(2, T - 3)
    rows = np.full((3, T), D - 1, dtype=np.int32)
    rows[0] = (2 + np.arange(T)) % m
    rows[1] = (1 + 2 * np.arange(T)) % m
    rows[2, :short] = (3 + np.arange(short) + (np.arange(short) > short // 2)) % m
    return rows, np.array([T, T, short], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _model(T, n, c, variant, b):
    rows, lens = _kernel_rows(T)
    X = _panel()[rows[b, :lens[b]], :n]
    assert gm.margin(X, c) >= MARGIN_MIN
    return gm.gerber(X, c, variant), X


def _run(pan, rd, td, c, variant, corr, out=None):
    B, n = rd.shape[0], pan.n
    ld = engine.round_up(n, 64)
    if out is None:
        out = torch.full((B, ld, ld), POISON, dtype=F64, device=pan.device)
    S, status, counts = engine.gerber_cov(pan, rd, td, threshold=c, variant=variant, corr=corr, out=out)
    assert S is out and status.dtype == torch.int32 and counts.dtype == torch.int32
    assert tuple(status.shape) == (B,) and tuple(counts.shape) == (B, ld)
    torch.cuda.synchronize()
    return S.cpu().numpy(), status.cpu().numpy(), counts.cpu().numpy()


# ---- 1. the kernels -----------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("c", THRESHOLDS)
@pytest.mark.parametrize("T,n", CASES)
def test_kernels_match_model(device, T, n, c, variant):
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    S, st, cnt = _run(pan, rd, td, c, variant, False)
    G, stg, cntg = _run(pan, rd, td, c, variant, True)
    assert list(st) == [OK] * 3 and list(stg) == [OK] * 3 and np.array_equal(cnt, cntg)
    worst = dict(g=0.0, sigma=0.0, diag=0.0)
    for b in range(3):
        mod, X = _model(T, n, c, variant, b)
        assert mod.status == gm.OK
        assert np.array_equal(cnt[b, :n], mod.a) and not cnt[b, n:].any()
        Gb, Sb = G[b, :n, :n], S[b, :n, :n]
        if variant == 1:
            assert np.array_equal(Gb, mod.G)                    # one IEEE division of two integers
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.where(mod.G != 0, np.abs(Gb - mod.G) / np.abs(mod.G), np.abs(Gb))
            worst["g"] = max(worst["g"], float(rel.max()))
        worst["sigma"] = max(worst["sigma"], float((np.abs(Sb - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
        var = X.var(axis=0, ddof=1)
        worst["diag"] = max(worst["diag"], float((np.abs(np.diag(Sb) - var) / var).max()))
        assert np.array_equal(Sb, Sb.T) and np.array_equal(Gb, Gb.T)
        for M in (S[b], G[b]):                                    # nothing outside [0, n) x [0, n)
            assert np.all(M[n:, :] == POISON) and np.all(M[:, n:] == POISON)
        # the date alone: the same bits
        S1, st1, cnt1 = _run(pan, rd[b:b + 1], td[b:b + 1], c, variant, False)
        assert st1[0] == OK and np.array_equal(S1[0], S[b]) and np.array_equal(cnt1[0], cnt[b])
    print(f"gerber (T, n) = {(T, n)} c = {c} variant {variant}: G {worst['g']:.2e}, Sigma {worst['sigma']:.2e}, "
          f"diag {worst['diag']:.2e}")
    assert worst["g"] <= G2_TOL
    assert worst["sigma"] <= SIGMA_TOL
    assert worst["diag"] <= SIGMA_TOL


def test_chunks_and_repeats_are_bitwise_equal(device):
    T, n = 65, 130
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    one = engine.gerber_cov(pan, rd, td)
    two = engine.gerber_cov(pan, rd, td, chunk_bytes=1)           # one date per chunk of the sign panel
    three = engine.gerber_cov(pan, rd, td)
    for a, b, c in zip(one, two, three):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not one[0][:, n:, :].any() and not one[0][:, :, n:].any()   # an allocated result: zero padding
    empty = engine.gerber_cov(pan, rd[:0], td[:0])
    assert empty[0].shape == (0, 192, 192) and empty[1].shape == (0,) and empty[2].shape == (0, 192)


# ---- 2. bad input -------------------------------------------------------------------------------

def test_bad_dates_do_not_affect_their_neighbours(device):
    """A constant column, a NaN, a one-row window and (at c = 1) a column alternating +-v, whose
    standard deviation exceeds v so that the asset never moves beyond its threshold, in one batch
    beside two good dates: BAD_INPUT and a NaN block each; the good dates' bits are their solo run's."""
    T, n, c = 17, 20, 1.0
    R = _panel()[:, :n].copy()
    R[100:100 + T, 3] = 0.25
    R[155, 2] = np.nan
    R[200:200 + T, 5] = 0.01 * (-1.0) ** np.arange(T)
    starts = [2, 100, 150, 40, 60, 200]
    rows = np.stack([s + np.arange(T) for s in starts]).astype(np.int32)
    lens = np.array([T, T, T, T, 1, T], dtype=np.int32)
    rows[4, 1:] = R.shape[0] - 1
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    for variant in (1, 2):
        S, st, cnt = _run(pan, rd, td, c, variant, False)
        assert list(st) == [OK, BAD, BAD, OK, BAD, BAD]
        for b in (1, 2, 4, 5):
            assert gm.gerber(R[rows[b, :lens[b]]], c, variant).status == gm.BAD_INPUT
            assert np.isnan(S[b, :n, :n]).all()
            assert np.all(S[b, n:, :] == POISON) and np.all(S[b, :, n:] == POISON)
        for b in (0, 3):
            X = R[rows[b]]
            mod = gm.gerber(X, c, variant)
            assert mod.status == gm.OK and gm.margin(X, c) >= MARGIN_MIN
            assert np.array_equal(cnt[b, :n], mod.a)
            assert float((np.abs(S[b, :n, :n] - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()) <= SIGMA_TOL
            S1, st1, _ = _run(pan, rd[b:b + 1], td[b:b + 1], c, variant, False)
            assert st1[0] == OK and np.array_equal(S1[0], S[b])


# ---- 3. host argument checks: an error, nothing launched ------------------------------------------

@pytest.mark.parametrize("kw", [{"tmax": _lib.PQ_GERBER_TMAX + 1}, {"variant": 3}, {"variant": 0}, {"threshold": 0.0},
                                {"threshold": 1.5}, {"threshold": float("nan")}, {"stages": 0}, {"stages": 4},
                                {"n": 0}, {"ld": 19}, {"null": "panel"}, {"null": "rows"}, {"null": "tlen"},
                                {"null": "dg"}, {"null": "St"}, {"null": "counts"}, {"null": "out"},
                                {"null": "status"}])
def test_host_argument_checks(device, kw):
    T, n = 17, 20
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    dg = pan.window_sumsq(rd, td, pan.window_means(rd, td))
    out = torch.full((3, 64, 64), POISON, dtype=F64, device=device)
    status = torch.full((3,), 7, dtype=torch.int32, device=device)
    counts = torch.full((3, 64), -7, dtype=torch.int32, device=device)
    St = torch.full((3, 64 * 64), 5, dtype=torch.int8, device=device)
    torch.cuda.synchronize()
    p = dict(panel=_ptr(pan.R), rows=_ptr(rd), tlen=_ptr(td), dg=_ptr(dg), St=_ptr(St), counts=_ptr(counts),
             out=_ptr(out), status=_ptr(status))
    kw = dict(kw)
    if "null" in kw:
        p[kw.pop("null")] = None
    rc = _lib.load().pq_gerber_cov_batched(
        p["panel"], pan.R.stride(0), kw.get("n", n), p["rows"], p["tlen"], kw.get("tmax", T), 3, p["dg"], dg.stride(0),
        kw.get("threshold", 0.5), kw.get("variant", 2), 0, kw.get("stages", 3), p["St"], p["counts"], 64, p["out"],
        kw.get("ld", 64), 64 * 64, p["status"], engine._stream())
    torch.cuda.synchronize()
    assert rc != 0 and _lib.load().pq_last_error()
    assert torch.all(out == POISON) and torch.all(status == 7) and torch.all(counts == -7) and torch.all(St == 5)
    for bad in ({"threshold": 0}, {"threshold": 1.5}, {"variant": 3}):
        with pytest.raises(ValueError, match="gerber"):
            engine.gerber_cov(pan, rd, td, **bad)
    with pytest.raises(ValueError, match="out must be"):
        engine.gerber_cov(pan, rd, td, out=out[:, :32])


# ---- 4. Covariance(method='gerber') ---------------------------------------------------------------

def _frame(n, D, seed=None):
    dates, R, _, _ = factor_panel(D, n, **({} if seed is None else {"seed": seed}))
    return pd.DataFrame(R, index=pd.DatetimeIndex(dates), columns=[f"A{i:03d}" for i in range(n)])


def test_covariance_estimate(device):
    X = _frame(12, 60)
    worst = 0.0
    for kw in ({}, {"threshold": 0.3, "variant": 1}, {"threshold": 0.9}):
        c, variant = kw.get("threshold", 0.5), kw.get("variant", 2)
        assert gm.margin(X.to_numpy(), c) >= MARGIN_MIN
        S = Covariance(method="gerber", check_positive_definite=False, **kw).estimate(X)
        assert isinstance(S, pd.DataFrame) and list(S.index) == list(X.columns) and list(S.columns) == list(X.columns)
        mod = gm.gerber(X.to_numpy(), c, variant)
        worst = max(worst, float((np.abs(S.to_numpy() - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
        assert np.array_equal(cov_gerber(X, c, variant).to_numpy(), S.to_numpy())
    print(f"Covariance.estimate: {worst:.2e}")
    assert worst <= SIGMA_TOL
    assert isinstance(cov_gerber(X.to_numpy()), np.ndarray)
    X2 = _frame(40, 30)                                           # more assets than rows: singular, repaired
    S2 = Covariance(method="gerber", check_positive_definite=True).estimate(X2)
    assert isinstance(S2, pd.DataFrame) and list(S2.columns) == list(X2.columns) and isPD(S2)
    Xn = X.copy()
    Xn.iloc[7, 3] = np.nan
    with pytest.raises(ValueError, match="complete windows"):
        Covariance(method="gerber").estimate(Xn)
    with pytest.raises(ValueError, match="bad input"):
        Covariance(method="gerber").estimate(pd.DataFrame(np.full((10, 6), 0.25)))


def test_estimate_batch_lr(device):
    T, n = 65, 130
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:-1, :n])
    rd, td = pan.rows_to_device(np.where(rows == 399, 0, rows), lens)
    cov = Covariance(method="gerber", threshold=0.3)
    out = torch.full((3, 192, 192), POISON, dtype=F64, device=device)
    S, pdiag, mu, dg = cov.estimate_batch_lr(pan, rd, td, out=out, materialise=True)
    assert S is out and mu is None and dg is None and torch.equal(pdiag, torch.zeros(3, dtype=F64, device=device))
    ref = engine.gerber_cov(pan, rd, td, threshold=0.3)[0]
    assert torch.equal(S, ref)                                    # the padding of a dense P is zero
    assert torch.equal(cov.estimate_batch(pan, rd, td)[0], ref)
    with pytest.raises(NotImplementedError, match="per date|own window"):
        cov.estimate_batch_lr(pan, rd, td, materialise=False)


# ---- 5. MeanVariance: the dense batched route ------------------------------------------------------

def _service(opt, X, rebdates, width, budget=1.0, upper=0.2):
    return BacktestService(
        data={"return_series": X},
        selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
        optimization_item_builders={
            "return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=budget),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, upper=upper)},
        optimization=opt, rebdates=rebdates, quiet=True)


def test_mean_variance_backtest(device):
    """'gerber' variant 2 on the dense batched route: every date against the oracle IPM on
    P = 2 ra Sigma_model (the bounds of tests/test_shrinkage_gpu.py::test_backtest_matches_oracle
    for the dense route); variant 1 completes through the serial loop."""
    from oracle.qp_ipm import solve_qp
    width, n, ra, ndates = 60, 12, 2.0, 6
    X = _frame(n, 100, seed=11)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + ndates]]
    opt = MeanVariance(covariance=Covariance(method="gerber"), solver_name="mi355x", risk_aversion=ra)
    bt = Backtest()
    bt.run(_service(opt, X, rebdates, width))
    assert bt.stats["solved"] == ndates and bt.stats["path"] == "dense"
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    Xv = X.to_numpy()
    for i, d in enumerate(rebdates):
        e = X.index.get_loc(pd.Timestamp(d))
        Xw = Xv[e - width + 1:e + 1]
        assert gm.margin(Xw, 0.5) >= MARGIN_MIN
        P = 2 * ra * gm.gerber(Xw, 0.5, 2).Sigma
        q = -rp.mean_geometric(Xw, None, None, None)
        o = solve_qp(P, q, A=np.ones((1, n)), b=np.ones(1), lb=np.zeros(n), ub=np.full(n, 0.2))
        obj = 0.5 * W[i] @ P @ W[i] + q @ W[i]
        assert abs(obj - o.obj) <= 1e-6 * max(abs(o.obj), 1e-12), (i, obj, o.obj)
        assert np.abs(W[i] - o.x).max() < 1e-5, (i, np.abs(W[i] - o.x).max())
        assert abs(W[i].sum() - 1) < 1e-7 and W[i].min() > -1e-7 and W[i].max() < 0.2 + 1e-7
    opt1 = MeanVariance(covariance=Covariance(method="gerber", variant=1), solver_name="mi355x", risk_aversion=ra)
    assert opt1.objective_batch(None) is None
    bt1 = Backtest()
    bt1.run(_service(opt1, X, rebdates, width))
    assert bt1.stats.get("path") is None                         # the serial loop
    W1 = bt1.strategy.get_weights_df().to_numpy(dtype=float)
    assert W1.shape == (ndates, n) and np.abs(W1.sum(axis=1) - 1.0).max() <= 1e-7


# ---- 6. HierarchicalRiskParity ----------------------------------------------------------------------

SCALE = 0.7


@pytest.mark.parametrize("linkage", ["single", "average"])
def test_hrp_on_the_gerber_matrix(device, linkage):
    """Gerber correlations take few distinct values, so merge distances tie and the tree is not
    comparable across implementations: the device's own tree is checked for consistency (its leaf
    order, the bisection of that order on the model's Sigma, the multiset of single-linkage merge
    distances), never against another tree."""
    n, T, ndates = 24, 100, 6
    X = _frame(n, 140, seed=11)
    rebdates = [str(d.date()) for d in X.index[T + 5:T + 5 + ndates]]

    def make():
        opt = HierarchicalRiskParity(covariance=Covariance(method="gerber"), linkage=linkage)
        opt.constraints = Constraints(selection=list(X.columns))
        opt.constraints.add_budget(rhs=SCALE)
        return opt
    worst = dict(x=0.0, link=0.0)
    solo = []
    for d in rebdates:
        e = X.index.get_loc(pd.Timestamp(d))
        win = X.iloc[e - T + 1:e + 1]
        assert gm.margin(win.to_numpy(), 0.5) >= MARGIN_MIN
        opt = make()
        opt.set_objective(OptimizationData(align=False, return_series=win))
        assert opt.solve() is True
        Z = opt.results["linkage"]
        order = np.array([X.columns.get_loc(a) for a in opt.results["order"]])
        assert np.array_equal(order, hm.leaves(Z, n))
        mod = gm.gerber(win.to_numpy(), 0.5, 2)
        xm = LD(SCALE) * hm.bisect(mod.Sigma.astype(LD), order)
        x = np.array([opt.results["weights"][a] for a in X.columns])
        worst["x"] = max(worst["x"], float(np.max(np.abs(x - xm) / xm)))
        assert abs(x.sum() - SCALE) <= 1e-14
        if linkage == "single":
            dm = np.sort(hm.prim_edges(hm.distance(mod.Sigma))[2])
            worst["link"] = max(worst["link"], float(np.abs(np.sort(Z[:, 2]) - dm).max()))
        solo.append(x)
    print(f"hrp on gerber ({linkage}): weights {worst['x']:.2e}, merge distances {worst['link']:.2e}")
    assert worst["x"] <= HRP_TOL and worst["link"] <= LINK_TOL
    bt = Backtest()
    bt.run(_service(make(), X, rebdates, T, budget=SCALE))
    assert bt.stats.get("path") == "hrp"
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    assert W.shape == (ndates, n) and np.array_equal(W, np.stack(solo))
    # a bad-input date arrives as NaN and is the kernel's own bad input: the date is named
    Xz = X.copy()
    Xz.iloc[:X.index.get_loc(pd.Timestamp(rebdates[2])) + 1, 4] = 0.25
    with pytest.raises(RuntimeError, match=rebdates[0] + ".*bad input"):
        Backtest().run(_service(make(), Xz, rebdates, T, budget=SCALE))


def test_hrp_weights_dense_hook_default_is_unchanged(device):
    n, T = 24, 60
    pan = engine.Panel(_panel()[:-1, :n])
    rd, td = pan.rows_to_device(*_kernel_rows_clean(T))
    base = engine.hrp_weights(pan, rd, td, linkage=True)
    hook = engine.hrp_weights(pan, rd, td, linkage=True, dense=lambda r, t, out: pan.cov(r, t, mode=0, out=out))
    for a, b in zip(base, hook):
        assert torch.equal(a, b)
    g = engine.hrp_weights(pan, rd, td, chunk_bytes=1,
                           dense=lambda r, t, out: engine.gerber_cov(pan, r, t, out=out)[0])
    assert torch.all(g[3] == _lib.PQ_HRP_OK) and float((g[0].sum(1) - 1.0).abs().max()) <= 1e-14


def _kernel_rows_clean(T):
    rows, lens = _kernel_rows(T)
    return np.where(rows == _panel().shape[0] - 1, 0, rows), lens


# ---- 7. what 'gerber' does not serve -----------------------------------------------------------------

def test_risk_parity_needs_a_window_form(device):
    X = _frame(12, 60)
    opt = RiskParity(covariance=Covariance(method="gerber"))
    opt.constraints = Constraints(selection=list(X.columns))
    opt.set_objective(OptimizationData(align=False, return_series=X))
    with pytest.raises(NotImplementedError):
        opt.solve()
