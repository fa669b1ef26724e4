"""pq_risk_parity_batched, engine.risk_parity_weights, RiskParity and its Backtest.run path
against the extended-precision model of tests/risk_parity_model.py.

Every kernel batch is the five-date row table of tests/test_shrinkage_gpu.py (full,
weekend-skipping, half, short and single-row windows, -1 padding) on a panel whose row pitch
is wider than n (the padding columns hold NaN: a read past n poisons the result).
"""
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
from porqua_amd.covariance import Covariance
from porqua_amd.optimization import RP_NAN_MESSAGE, RiskParity
from porqua_amd.synthetic import factor_panel
from tests import risk_parity_model as m
from tests import shrinkage_model as sm
from tests.test_shrinkage_gpu import _row_table

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
U = 2.0 ** -53
EPS = 1e-10
RIDGE = 2e-5        # the c > 0 cases (the assets' variances are about 5e-4)
PAD = 3             # panel row pitch = n + PAD
# |y_k(float64, blocked) - y_k(model)| / y_k(model) of the float64 numpy restatement
# (risk_parity_model.blocked_f64, window centred in float64) for k in {1, 2, 5} over every case,
# budget and date with a positive diagonal below, measured on the CPU: at most 2.56e-14 (n = 130,
# the uncentred single-row date, Sigma of rank one: the short windows amplify rounding most;
# 1.6e-15 on the full windows, 1.4e-14 on the (1000, 252) case).  The bound is 10x the largest.
# (The kernel itself, on MI355X: at most 4.3e-14, on the three-row date of the (1000, 252) case.)
ITER_TOL = 2.6e-13
OK, MAXS, BAD = _lib.PQ_RP_OK, _lib.PQ_RP_MAX_SWEEPS, _lib.PQ_RP_BAD_INPUT

PAIRS = [(1, 2), (2, 3), (5, 7), (15, 63), (16, 64), (17, 65), (37, 252), (130, 257), (130, 63), (37, 7)]
BUDGETS = {"equal": m.equal_budget, "skewed": m.skewed_budget}


@functools.lru_cache(maxsize=None)
def _panel(n):
    return factor_panel(1100, n)[1]


class Case:
    """One five-date batch: host data and the model's Sigma per date (None: Sigma has a
    non-positive diagonal entry, the date is bad input)."""

    def __init__(self, n, T, centred, c, R=None):
        self.n, self.T, self.centred = n, T, centred
        self.R = _panel(n) if R is None else R
        self.rows, self.lens = _row_table(T)
        B = len(self.lens)
        self.a = 1.0 / np.maximum(self.lens - 1, 1).astype(np.float64)
        self.c = np.full(B, float(c))
        self.X = [m.window(self.R, self.rows[d, :self.lens[d]], centred) for d in range(B)]
        self.S = []
        for d in range(B):
            S = m.sigma(self.X[d], self.a[d], self.c[d])
            self.S.append(S if np.all(np.diag(S) > 0) and np.all(np.isfinite(np.asarray(S, dtype=np.float64))) else None)

    def good(self):
        return [d for d in range(len(self.lens)) if self.S[d] is not None]


@functools.lru_cache(maxsize=None)
def _case(n, T, centred, ridge):
    return Case(n, T, centred, RIDGE if ridge else 0.0)


def _launch(case, budget, eps=EPS, max_sweeps=500, scale=1.0, dates=None, R=None, tmax=None, ldb=None, ldx=None):
    """The kernel on ``dates`` (default: all five) of the case; mu and dg come from torch, in
    float64, on the device.  ``budget``: (n,) shared or (B, n).  Returns (rc, x, stats, status)
    as numpy; outputs are pre-filled with -7 so that a call that does not launch shows."""
    lib = _lib.load()
    dev = engine.default_device()
    n = case.n
    dates = list(range(len(case.lens))) if dates is None else list(dates)
    B = len(dates)
    Rh = case.R if R is None else R
    Rp = np.full((Rh.shape[0], n + PAD), np.nan)
    Rp[:, :n] = Rh
    Rd = torch.from_numpy(Rp).to(dev)
    rows = np.ascontiguousarray(case.rows[dates])
    lens = np.ascontiguousarray(case.lens[dates])
    rows_d, tlen_d = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    ld = engine.round_up(n, 64)
    mu = torch.zeros((B, ld), dtype=F64, device=dev)
    dg = torch.zeros((B, ld), dtype=F64, device=dev)
    for i in range(B):
        Xw = Rd[torch.from_numpy(rows[i, :lens[i]].astype(np.int64)).to(dev), :n]
        if case.centred:
            mu[i, :n] = Xw.mean(dim=0)
            Xw = Xw - mu[i, :n]
        dg[i, :n] = (Xw * Xw).sum(dim=0)
    a_d = torch.from_numpy(case.a[dates]).to(dev)
    c_d = torch.from_numpy(case.c[dates]).to(dev)
    bud = torch.from_numpy(np.ascontiguousarray(np.asarray(budget, dtype=np.float64).reshape(-1, n))).to(dev)
    if ldb is None:
        ldb = 0 if bud.shape[0] == 1 else n
    ldx_alloc = n + 1
    x = torch.full((B, ldx_alloc), -7.0, dtype=F64, device=dev)
    stats = torch.full((B, 4), -7.0, dtype=F64, device=dev)
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    lr = _lib.PQLowRank(panel=Rd.data_ptr(), ldp=Rd.stride(0), rows=rows_d.data_ptr(), tlen=tlen_d.data_ptr(),
                        tmax=case.T if tmax is None else tmax, mu=mu.data_ptr() if case.centred else None,
                        mu_stride=ld if case.centred else 0, w_scale=None, dg=dg.data_ptr(), dg_stride=ld)
    rc = lib.pq_risk_parity_batched(ctypes.byref(lr), n, B, a_d.data_ptr(), c_d.data_ptr(), bud.data_ptr(), ldb,
                                    float(scale), float(eps), int(max_sweeps), x.data_ptr(),
                                    ldx_alloc if ldx is None else ldx, stats.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    assert rc != 0 or np.all(xh[:, n] == -7.0)          # nothing written past n
    return rc, xh[:, :n], stats.cpu().numpy(), status.cpu().numpy()


def _assert_bad(x, stats, status, d):
    assert status[d] == BAD and np.all(np.isnan(x[d])) and np.all(np.isnan(stats[d]))


# ---- iterates ---------------------------------------------------------------------------------

def _check_iterates(case, bname, ks=(1, 2, 5)):
    b = BUDGETS[bname](case.n)
    worst = 0.0
    for k in ks:
        rc, x, stats, status = _launch(case, b, eps=0.0, max_sweeps=k)
        assert rc == 0
        for d in range(len(case.lens)):
            if case.S[d] is None:
                _assert_bad(x, stats, status, d)
                continue
            assert stats[d, 1] == k and status[d] in (OK, MAXS)
            assert (status[d] == OK) == (stats[d, 0] <= 0.0)
            y = x[d].astype(LD) * LD(stats[d, 3])
            ref = m.iterate(case.S[d], b, k)
            err = float(np.max(np.abs(y - ref) / ref))
            worst = max(worst, err)
            print(f"iterate n={case.n} T={case.T} {bname} k={k} date={d}: rel err {err:.2e}")
            assert err <= ITER_TOL, (k, d, err)
    return worst


@pytest.mark.parametrize("ridge", [False, True])
@pytest.mark.parametrize("centred", [True, False])
@pytest.mark.parametrize("n,T", PAIRS)
def test_iterates_match_model(device, n, T, centred, ridge):
    """eps = 0, max_sweeps = k: y = x * stats[3] is the model's k-th iterate (ordered,
    Gauss-Seidel: a Jacobi-style or mis-ordered update differs in the first digits)."""
    case = _case(n, T, centred, ridge)
    for bname in BUDGETS:
        _check_iterates(case, bname)


# ---- optimum ----------------------------------------------------------------------------------

def _residual_bar(case, d, b, y):
    """A bound on what evaluating max_i |y_i (Sigma y)_i - b_i| / b_i in float64 can differ from
    the exact value, from the absolute terms: r_t = sum_j x_tj y_j is an n-term sum, (Sigma y)_i
    a T-term sum over it (any summation order), plus a few roundings of the scalars."""
    Xa = np.abs(case.X[d])
    y = np.asarray(y, dtype=LD)
    r = case.X[d] @ y
    a, c = LD(case.a[d]), LD(case.c[d])
    n, T = case.n, case.lens[d]
    s_abs = a * (n * (Xa.T @ (Xa @ y)) + T * (Xa.T @ np.abs(r))) + 8 * (a * np.abs(case.X[d].T @ r) + c * y)
    return float(np.max(y * s_abs / np.asarray(b, dtype=LD) + 8) * U)


def _check_optimum(case, bname):
    b = BUDGETS[bname](case.n)
    rc, x, stats, status = _launch(case, b)
    assert rc == 0
    for d in range(len(case.lens)):
        S = case.S[d]
        if S is None:
            _assert_bad(x, stats, status, d)
            continue
        assert np.all(np.isfinite(x[d])) and np.all(x[d] > 0) and abs(x[d].sum() - 1.0) <= 4 * case.n * U
        # the record: res, x' Sigma x, sum y of the returned x against the model (1e-9 relative;
        # for res on top of the float64 evaluation's own rounding, which 1e-9 of a residual of
        # 1e-11 cannot hold: the terms y_i (Sigma y)_i / b_i it is the difference of are near 1)
        res_m, var_m, sumy_m = m.record(S, b, x[d], stats[d, 3])
        y = x[d].astype(LD) * LD(stats[d, 3])
        print(f"optimum n={case.n} T={case.T} {bname} date={d}: status {status[d]} sweeps {stats[d, 1]:.0f} "
              f"res {stats[d, 0]:.3e} model {res_m:.3e} bar {_residual_bar(case, d, b, y):.1e}")
        assert abs(stats[d, 0] - res_m) <= 1e-9 * res_m + _residual_bar(case, d, b, y), (d, stats[d, 0], res_m)
        assert abs(stats[d, 2] - var_m) <= 1e-9 * var_m and abs(stats[d, 3] - sumy_m) <= 1e-9 * sumy_m
        assert (status[d] == OK) == (stats[d, 0] <= EPS) and status[d] in (OK, MAXS)
        assert stats[d, 1] <= 500 and (status[d] == OK or stats[d, 1] == 500)
        # well-posed: the model itself converges to 1e-10 within 100 sweeps (the short windows
        # with fewer rows than assets need thousands, or have no optimum at all)
        _, k10, r10 = m.solve(S, b, eps=EPS, max_sweeps=100)
        if r10 > EPS:
            continue
        assert status[d] == OK, (d, stats[d])
        assert res_m <= 10 * EPS
        yopt, _, ropt = m.solve(S, b, eps=1e-14, max_sweeps=400)
        assert ropt <= 1e-14
        xopt = m.weights(yopt)
        err = float(np.max(np.abs(x[d] - xopt) / xopt))
        print(f"    model sweeps(1e-10) {k10}; x rel err {err:.2e} (bound {2 * EPS / np.sqrt(b.min()):.1e})")
        assert err <= 2 * EPS / np.sqrt(b.min()), (d, err)


@pytest.mark.parametrize("ridge", [False, True])
@pytest.mark.parametrize("centred", [True, False])
@pytest.mark.parametrize("n,T", PAIRS)
def test_optimum_matches_model(device, n, T, centred, ridge):
    """Defaults (eps 1e-10, 500 sweeps): every well-posed date is PQ_RP_OK; its residual recomputed
    in longdouble from x is <= 10 eps; x is within 2 eps / sqrt(min b) of the model's optimum
    (H >= diag(b / y^2), so sum_i b_i (dy_i / y_i)^2 <= res^2, and normalising doubles it); the
    stats agree with the model's values for the returned x.  The single-row centred date without a
    ridge has Sigma = 0: PQ_RP_BAD_INPUT."""
    case = _case(n, T, centred, ridge)
    if centred and not ridge:
        assert case.S[4] is None
    for bname in BUDGETS:
        _check_optimum(case, bname)


def test_thousand_assets(device):
    """(n, T) = (1000, 252): 63 tiles, the k = 2 iterate and the optimum."""
    case = _case(1000, 252, True, False)
    _check_iterates(case, "equal", ks=(2,))
    _check_optimum(case, "equal")


# ---- failure modes ------------------------------------------------------------------------------

def _others_unchanged(case, budget, bad_date, full, R=None, **kw):
    """The dates other than ``bad_date`` are bitwise what the batch without it gives."""
    keep = [d for d in range(len(case.lens)) if d != bad_date]
    bsub = budget if np.ndim(budget) == 1 else np.asarray(budget)[keep]
    rc, x, stats, status = _launch(case, bsub, dates=keep, R=R, **kw)
    assert rc == 0
    _, xf, sf, stf = full
    assert np.array_equal(xf[keep], x, equal_nan=True) and np.array_equal(sf[keep], stats, equal_nan=True)
    assert np.array_equal(stf[keep], status)


@pytest.mark.parametrize("value", [0.0, -0.05, float("nan"), float("inf")])
def test_bad_budget_entry(device, value):
    case = _case(17, 65, True, True)
    bud = np.tile(m.skewed_budget(17), (5, 1))
    bud[1, 16] = value
    full = _launch(case, bud)
    assert full[0] == 0
    _assert_bad(*full[1:], 1)
    assert all(full[3][d] == OK for d in (0, 2)) and np.all(np.isfinite(full[1][[0, 2, 3, 4]]))
    _others_unchanged(case, bud, 1, full)


def test_nan_in_one_window(device):
    case = _case(17, 65, True, True)
    # a row of the full window that no other date reads (the weekend pattern skips it)
    others = set(np.concatenate([case.rows[d, :case.lens[d]] for d in (1, 2, 3, 4)]).tolist())
    row = next(int(r) for r in case.rows[0, :case.lens[0]] if int(r) not in others)
    R = case.R.copy()
    R[row, 5] = np.nan
    b = m.equal_budget(17)
    full = _launch(case, b, R=R)
    assert full[0] == 0
    _assert_bad(*full[1:], 0)
    _others_unchanged(case, b, 0, full, R=R)
    clean = _launch(case, b)
    keep = [1, 2, 3, 4]
    assert np.array_equal(clean[1][keep], full[1][keep]) and np.array_equal(clean[2][keep], full[2][keep])


def test_zero_variance_column_without_ridge(device):
    base = _case(17, 65, True, False)
    R = base.R.copy()
    R[base.rows[2, :base.lens[2]], 9] = 0.015625    # constant over the half window (2^-6: sums stay exact)
    case = Case(17, 65, True, 0.0, R=R)
    assert case.S[2] is None and case.S[0] is not None
    b = m.equal_budget(17)
    full = _launch(case, b)
    assert full[0] == 0
    _assert_bad(*full[1:], 2)
    assert full[3][0] == OK and full[3][4] == BAD    # (the single-row date: Sigma = 0)
    _others_unchanged(case, b, 2, full)


def test_unbounded_problem_hits_max_sweeps(device):
    """x_2 = -x_1 exactly after centring, no ridge: y = (t, t, 0) is a positive null vector of
    Sigma, the objective has no minimiser.  50 sweeps: PQ_RP_MAX_SWEEPS, a finite x, an honest
    residual above eps."""
    T = 65
    rows, lens = _row_table(T)
    R = _panel(3).copy()
    w1 = rows[1, :lens[1]]
    R[w1, 1] = -R[w1, 0]
    case = Case(3, T, True, 0.0, R=R)
    Xc = np.asarray(case.X[1], dtype=np.float64)
    assert np.array_equal(Xc[:, 1], -Xc[:, 0])
    b = m.equal_budget(3)
    full = _launch(case, b, max_sweeps=50)
    rc, x, stats, status = full
    assert rc == 0 and status[1] == MAXS and stats[1, 1] == 50
    assert np.all(np.isfinite(x[1])) and np.all(np.isfinite(stats[1])) and stats[1, 0] > EPS
    res_m, _, _ = m.record(case.S[1], b, x[1], stats[1, 3])
    y = x[1].astype(LD) * LD(stats[1, 3])
    assert abs(stats[1, 0] - res_m) <= 1e-9 * res_m + _residual_bar(case, 1, b, y)
    _others_unchanged(case, b, 1, full, max_sweeps=50)


def test_identical_calls_are_bitwise_equal(device):
    case = _case(130, 257, True, False)
    b = m.skewed_budget(130)
    one, two = _launch(case, b), _launch(case, b)
    for p, q in zip(one[1:], two[1:]):
        assert np.array_equal(p, q, equal_nan=True)


@pytest.mark.parametrize("kw", [{"tmax": 0}, {"tmax": 1025}, {"ldb": -1}, {"ldx": 16}])
def test_host_argument_checks(device, kw):
    case = _case(17, 65, True, True)
    rc, x, stats, status = _launch(case, m.equal_budget(17), **kw)
    assert rc != 0 and _lib.load().pq_last_error()
    assert np.all(x == -7.0) and np.all(stats == -7.0) and np.all(status == -7)   # nothing launched


# ---- engine / API -----------------------------------------------------------------------------

def _frame(n, D, seed=11):
    dates, R, _, _ = factor_panel(D, n, seed=seed)
    return pd.DataFrame(R, index=pd.DatetimeIndex(dates), columns=[f"A{i:03d}" for i in range(n)])


def _solve_one(opt, X, budget=None):
    from porqua_amd.constraints import Constraints
    from porqua_amd.optimization_data import OptimizationData
    opt.constraints = Constraints(selection=list(X.columns))
    if budget is not None:
        opt.constraints.add_budget(rhs=budget)
    opt.constraints.add_box(box_type="LongOnly", upper=0.01)     # ignored: long-only by construction
    opt.set_objective(OptimizationData(align=False, return_series=X))
    ok = opt.solve()
    return ok, np.array([opt.results["weights"][k] for k in X.columns], dtype=np.float64)


def test_engine_defaults_and_empty_batch(device):
    n, T = 37, 63
    pan = engine.Panel(_panel(n))
    rows, lens = _row_table(T)
    rd, td = pan.rows_to_device(rows, lens)
    x, stats, status = engine.risk_parity_weights(pan, rd, td)
    assert x.is_cuda and stats.is_cuda and status.is_cuda and x.shape == (5, n) and stats.shape == (5, 4)
    st = status.cpu().numpy()
    assert list(st[:3]) == [OK] * 3 and st[4] == BAD              # one row: no sample covariance
    b = m.equal_budget(n)
    for d in range(3):
        S = m.sigma(m.window(_panel(n), rows[d, :lens[d]]), 1.0 / (lens[d] - 1), 0.0)
        assert m.residual(S, b, x[d].cpu().numpy().astype(LD) * LD(stats[d, 3].item())) <= 10 * EPS
    xe, se, ste = engine.risk_parity_weights(pan, rd[:0], td[:0])
    assert xe.shape == (0, n) and se.shape == (0, 4) and ste.shape == (0,)


def test_solve_matches_engine_bitwise(device):
    X = _frame(24, 80).iloc[5:65]
    opt = RiskParity()
    ok, w = _solve_one(opt, X)
    assert ok and opt.results["status"] is True
    pan = engine.Panel(X.to_numpy())
    rd, td = pan.rows_to_device(np.arange(60, dtype=np.int32)[None], np.array([60], dtype=np.int32))
    x, _, status = engine.risk_parity_weights(pan, rd, td)
    assert int(status[0].item()) == OK and np.array_equal(w, x[0].cpu().numpy())
    rc = np.array([opt.results["risk_contributions"][k] for k in X.columns])
    assert np.abs(rc * 24 - 1).max() <= 10 * EPS


@pytest.mark.parametrize("method", ["pearson", "linear_shrinkage", "ledoit_wolf", "oas", "duv"])
def test_risk_contributions_equal_budget_for_every_covariance(device, method):
    """x_i (Sigma x)_i / x' Sigma x against the budget, Sigma from the oracle's covariance in
    numpy (ledoit_wolf / oas: the oracle's sample covariance shrunk by the model's intensity)."""
    X = _frame(24, 80).iloc[5:65]
    Xv = X.to_numpy()
    n = Xv.shape[1]
    kw = {"lambda_covmat_regularization": 0.3} if method == "linear_shrinkage" else {}
    if method == "pearson":
        S = rp.cov_pearson(Xv)
    elif method == "linear_shrinkage":
        S = rp.cov_linear_shrinkage(Xv, 0.3)
    elif method == "duv":
        S = rp.cov_duv(Xv)
    else:
        delta = float(sm.stats(Xv, method)[3])
        S0 = rp.cov_pearson(Xv)
        S = (1 - delta) * S0 + delta * np.mean(np.diag(S0)) * np.eye(n)
    bud = {k: 1.0 + (i % 5) for i, k in enumerate(X.columns)}
    bud["NOT_SELECTED"] = 100.0                                    # normalised over the selection only
    opt = RiskParity(covariance=Covariance(method=method, **kw), risk_budget=bud)
    ok, w = _solve_one(opt, X)
    assert ok and abs(w.sum() - 1) <= 1e-14 and w.min() > 0
    b = np.array([bud[k] for k in X.columns])
    b = b / b.sum()
    rc = np.asarray(m.risk_contributions(S, w), dtype=np.float64)
    assert np.abs(rc / b - 1).max() <= 10 * EPS
    got = np.array([opt.results["risk_contributions"][k] for k in X.columns])
    assert np.abs(got / b - 1).max() <= 10 * EPS


def test_budget_rhs_scales_and_missing_budget_raises(device):
    X = _frame(24, 80).iloc[5:65]
    _, w1 = _solve_one(RiskParity(), X)
    _, w7 = _solve_one(RiskParity(), X, budget=0.7)
    assert abs(w7.sum() - 0.7) <= 1e-14 and np.abs(w7 / (0.7 * w1) - 1).max() <= 8 * U
    with pytest.raises(ValueError, match="no entry"):
        _solve_one(RiskParity(risk_budget={"A000": 1.0}), X)
    with pytest.raises(ValueError, match="> 0"):
        _solve_one(RiskParity(risk_budget={k: 0.0 for k in X.columns}), X)
    Xn = X.copy()
    Xn.iloc[7, 3] = np.nan
    with pytest.raises(ValueError, match="missing values"):
        _solve_one(RiskParity(), Xn)


def _service(opt, X, rebdates, width, budget=1):
    return BacktestService(
        data={"return_series": X},
        selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
        optimization_item_builders={
            "return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=budget),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, upper=0.1)},
        optimization=opt, rebdates=rebdates, quiet=True)


def test_backtest_batched_equals_serial(device):
    width, n = 60, 40
    X = _frame(n, 160)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + 12]]
    bud = {k: 1.0 + (i % 3) for i, k in enumerate(X.columns)}
    W = []
    for batched in (True, False):
        opt = RiskParity(covariance=Covariance(method="ledoit_wolf"), risk_budget=bud)
        bs = _service(opt, X, rebdates, width, budget=0.7)
        bs.settings["batched"] = batched
        bt = Backtest()
        bt.run(bs)
        assert len(bt.strategy.portfolios) == len(rebdates)
        assert [p.rebalancing_date for p in bt.strategy.portfolios] == rebdates
        if batched:
            assert bt.stats["path"] == "risk_parity" and bt.stats["solved"] == len(rebdates)
            assert np.all(bt.stats["status"] == OK) and bt.stats["sweeps"].max() <= 500
        else:
            assert bt.stats.get("path") != "risk_parity"
        W.append(bt.strategy.get_weights_df().to_numpy(dtype=float))
        assert set(opt.results) == {"weights", "status", "risk_contributions"} and opt.results["status"] is True
    assert W[0].shape == (12, n) and np.abs(W[0].sum(axis=1) - 0.7).max() <= 1e-14
    # the same kernel on the same windows: the serial loop's weights are the batched run's, up to
    # what an intensity rounded differently may move two eps-accurate solves apart (each is within
    # 2 eps / sqrt(min b) of its optimum, test_optimum_matches_model)
    bmin = 1.0 / sum(bud.values())
    print("batched vs serial: max rel diff", np.abs(W[0] / W[1] - 1).max())
    assert np.abs(W[0] / W[1] - 1).max() <= 4 * EPS / np.sqrt(bmin)
    # and they are risk-budget portfolios of each date's Ledoit-Wolf covariance
    b = np.array([bud[k] for k in X.columns])
    b /= b.sum()
    Xv = X.to_numpy()
    for i in (0, 11):
        e = X.index.get_loc(pd.Timestamp(rebdates[i]))
        win = Xv[e - width + 1:e + 1]
        delta = float(sm.stats(win, "ledoit_wolf")[3])
        S0 = rp.cov_pearson(win)
        S = (1 - delta) * S0 + delta * np.mean(np.diag(S0)) * np.eye(n)
        assert np.abs(np.asarray(m.risk_contributions(S, W[0][i]), dtype=np.float64) / b - 1).max() <= 10 * EPS


def test_backtest_nan_panel_and_failed_date_raise(device):
    width, n = 60, 40
    X = _frame(n, 160)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + 12]]
    Xn = X.copy()
    Xn.iloc[40, 2] = np.nan
    for batched in (True, False):
        bs = _service(RiskParity(), Xn, rebdates, width)
        bs.settings["batched"] = batched
        with pytest.raises(RuntimeError, match="missing values"):
            Backtest().run(bs)
    assert "missing values" in RP_NAN_MESSAGE
    # a date that is not PQ_RP_OK raises, naming the date and the reason
    Xz = X.copy()
    e = X.index.get_loc(pd.Timestamp(rebdates[3]))
    Xz.iloc[:, 7] = 0.0
    Xz.iloc[e + 1:, 7] = X.iloc[e + 1:, 7]             # zero variance in every window up to date 3
    with pytest.raises(RuntimeError, match=rebdates[0] + ".*bad input"):
        Backtest().run(_service(RiskParity(), Xz, rebdates, width))
    one = _service(RiskParity(max_sweeps=1), X, rebdates, width)
    with pytest.raises(RuntimeError, match=rebdates[0] + ".*max_sweeps"):
        Backtest().run(one)
