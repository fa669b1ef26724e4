"""Ledoit-Wolf / OAS shrinkage on the device, layer by layer: pq_shrink_stats_band against the
longdouble model (tests/shrinkage_model.py), its conditioning, determinism and argument
checks; Covariance(method='ledoit_wolf' | 'oas') per window; Backtest.run on the window and the
dense route against the oracle IPM; the MinVarianceBacktest(shrinkage=...) workload hook."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import ref_pipeline as rp
from porqua_amd import _lib, engine
from porqua_amd.backtest import Backtest, BacktestService
from porqua_amd.builders import (OptimizationItemBuilder, SelectionItemBuilder, bibfn_box_constraints,
                                 bibfn_bm_series, bibfn_budget_constraint, bibfn_return_series,
                                 bibfn_selection_data)
from porqua_amd.covariance import Covariance, cov_ledoit_wolf, cov_oas
from porqua_amd.optimization import MeanVariance
from porqua_amd.synthetic import factor_panel
from porqua_amd.workloads import MinVarianceBacktest
from tests import shrinkage_model as sm

pytestmark = pytest.mark.gpu

F64 = torch.float64
KIND_ID = {"ledoit_wolf": 0, "oas": 1}
R0 = 5          # first band row (r0 > 0)
BASE = 9        # first panel row a window touches


@functools.lru_cache(maxsize=None)
def _panel(n):
    return factor_panel(1100, n)[1]


def _row_table(T):
    """Five dates with tmax = T: the full window; a weekend pattern (every 6th and 7th panel
    row dropped); a half window; a short one; a single row.  Padding is -1."""
    lens = [T, min(T, max(2, 2 * T // 3)), max(1, T // 2), min(T, 3), 1]
    starts = [BASE, BASE + 2, BASE + 11, BASE + 1, BASE + 30]
    rows = np.full((5, T), -1, dtype=np.int32)
    for d, (L, s) in enumerate(zip(lens, starts)):
        if d == 1:
            rows[d, :L] = [r for r in range(s, s + 2 * L + 14) if r % 7 not in (5, 6)][:L]
        else:
            rows[d, :L] = np.arange(s, s + L)
    return rows, np.array(lens, dtype=np.int32)


def _band_gram(lib, Rd, n, r0, nrows, W, ldo):
    """pq_lr_band_gram into a NaN-filled buffer: an entry the Gram does not define stays NaN."""
    band = torch.full((nrows, ldo), float("nan"), dtype=F64, device=Rd.device)
    _lib.check(lib.pq_lr_band_gram(Rd.data_ptr(), Rd.stride(0), n, r0, nrows, W, band.data_ptr(), ldo,
                                   None, 0, 0, None, 0, None), "pq_lr_band_gram")
    return band


def _stats_call(lib, band, ldo, r0, nrows, W, rows_d, tlen_d, tmax, n, centred, kind, ld_rows=None):
    B = int(tlen_d.shape[0])
    stats = torch.full((B, 4), -7.0, dtype=F64, device=band.device)
    rc = lib.pq_shrink_stats_band(band.data_ptr(), ldo, r0, nrows, W, rows_d.data_ptr(),
                                  rows_d.stride(0) if ld_rows is None else ld_rows, tlen_d.data_ptr(), tmax, B,
                                  n, centred, kind, stats.data_ptr(), None)
    return rc, stats


class _Setup:
    """Band Gram and row table of one (T, n) case, W strictly wider than the widest window."""

    def __init__(self, device, T, n):
        self.T, self.n = T, n
        self.R = _panel(n)
        self.rows, self.tlen = _row_table(T)
        last = np.array([self.rows[d, L - 1] for d, L in enumerate(self.tlen)])
        self.span = int((last - self.rows[:, 0] + 1).max())
        self.W = self.span + 5
        self.ldo = self.W + 3
        self.nrows = int(last.max()) - R0 + 1 + 3
        assert R0 + self.nrows <= self.R.shape[0] and np.ptp(self.rows[1, :self.tlen[1]]) + 1 > self.tlen[1]
        self.lib = _lib.load()
        self.Rd = torch.from_numpy(self.R).to(device)
        self.rows_d = torch.from_numpy(self.rows).to(device)
        self.tlen_d = torch.from_numpy(self.tlen).to(device)
        self.band = _band_gram(self.lib, self.Rd, n, R0, self.nrows, self.W, self.ldo)

    def call(self, centred, kind, **over):
        a = dict(band=self.band, ldo=self.ldo, r0=R0, nrows=self.nrows, W=self.W, rows_d=self.rows_d,
                 tlen_d=self.tlen_d, tmax=self.T, n=self.n, centred=centred, kind=KIND_ID[kind])
        a.update(over)
        return _stats_call(self.lib, **a)

    def window(self, d):
        return self.R[self.rows[d, :self.tlen[d]]]


CASES = ([(T, n) for T in (2, 3, 7, 63, 64, 65) for n in (5, 64, 130, 1000)]
         + [(T, n) for T in (252, 257, 1024) for n in (130, 1000)])


@pytest.mark.parametrize("T,n", CASES)
def test_stats_match_the_longdouble_model(device, T, n):
    """a, f, g to 1e-12 relative and delta to 1e-12 absolute (the project's moment tolerance),
    both kinds, centred and uncentred; mixed tlen, -1 padding, r0 > 0, W wider than any window
    and a date that skips panel rows in every batch."""
    su = _Setup(device, T, n)
    for centred in (1, 0):
        sums = [sm.stats(su.window(d), "ledoit_wolf", bool(centred))[:3] for d in range(5)]   # shared by both kinds
        model = {k: [s + (sm.delta_from(*s, su.tlen[d], n, k),) for d, s in enumerate(sums)] for k in sm.KINDS}
        for kind in sm.KINDS:
            rc, stats = su.call(centred, kind)
            assert rc == 0, su.lib.pq_last_error()
            got = stats.cpu().numpy()
            for d in range(5):
                m = model[kind][d]
                for k, name in enumerate("afg"):
                    err = abs(sm.LD(got[d, k]) - m[k])
                    assert err <= 1e-12 * abs(m[k]), (T, n, centred, kind, d, name, got[d, k], float(m[k]))
                assert abs(sm.LD(got[d, 3]) - m[3]) <= 1e-12, (T, n, centred, kind, d, got[d, 3], float(m[3]))
            if centred:   # a single row: a = f = g = 0 exactly
                assert np.array_equal(got[4], [0.0, 0.0, 0.0, 0.0 if kind == "ledoit_wolf" else 1.0])


def test_conditioning_large_mean(device):
    """Window 1.0 + N(0, 0.02^2), T = 252, n = 300, seed 1: the mean is 50 sigma, so centring
    from the uncentred Gram's row sums cancels about 3.5 digits.  The bound is 8 x the delta
    error of the float64 restatement of that algorithm (shrinkage_model.band_stats_f64) against
    the longdouble model on this exact input, computed here (8: another summation order).  On
    the CPU the restatement's error is 4.8e-13 (delta = 0.98344), so the bound is 3.8e-12."""
    X = 1.0 + np.random.default_rng(1).normal(0.0, 0.02, (252, 300))
    model = sm.stats(X, "ledoit_wolf")
    restated = sm.band_stats_f64(X, "ledoit_wolf")
    bound = 8.0 * abs(float(sm.LD(restated[3]) - model[3]))
    pan = engine.Panel(X, device=device)
    rows, tlen = pan.rows_to_device(np.arange(252, dtype=np.int32)[None], np.array([252], dtype=np.int32))
    delta, stats = engine.shrinkage_intensity(pan, rows, tlen, kind="ledoit_wolf")
    err = abs(float(sm.LD(delta.item()) - model[3]))
    print(f"conditioning: delta model {float(model[3]):.15f} gpu {delta.item():.15f} "
          f"restated {float(restated[3]):.15f} err {err:.3e} bound {bound:.3e}")
    assert 0.0 < float(model[3]) < 1.0
    assert err <= bound, (err, bound)


def test_stats_are_deterministic(device):
    su = _Setup(device, 252, 130)
    for kind in sm.KINDS:
        rc1, s1 = su.call(1, kind)
        rc2, s2 = su.call(1, kind)
        assert rc1 == 0 and rc2 == 0
        assert torch.equal(s1, s2)
        assert bool(torch.isfinite(s1).all())


def test_argument_rejections(device):
    """Every rejection returns an error with a message and faults nothing; a refused date's
    stats are NaN and the other dates of the batch are still computed."""
    su = _Setup(device, 65, 64)
    lib = su.lib
    rc, good = su.call(1, "ledoit_wolf")
    assert rc == 0

    def rejected(what, **over):
        rc, stats = su.call(1, "ledoit_wolf", **over)
        msg = lib.pq_last_error().decode()
        assert rc != 0 and what in msg, (what, rc, msg)
        torch.cuda.synchronize()
        return stats.cpu().numpy()

    rejected("tmax", tmax=1025, ld_rows=1025)
    st = rejected("spans more than W", W=su.span - 1)
    spans = np.array([su.rows[d, L - 1] - su.rows[d, 0] + 1 for d, L in enumerate(su.tlen)])
    assert np.isnan(st[spans > su.span - 1]).all() and np.isfinite(st[spans <= su.span - 1]).all()
    rows = su.rows.copy()
    rows[2, 0] = R0 - 1
    st = rejected("outside [r0", rows_d=torch.from_numpy(rows).to(device))
    assert np.isnan(st[2]).all() and np.array_equal(st[[0, 1, 3, 4]], good.cpu().numpy()[[0, 1, 3, 4]])
    rows = su.rows.copy()
    rows[0, 7] = rows[0, 6]
    rejected("increasing", rows_d=torch.from_numpy(rows).to(device))
    tlen = su.tlen.copy()
    tlen[3] = 0
    st = rejected("window length", tlen_d=torch.from_numpy(tlen).to(device))
    assert np.isnan(st[3]).all()
    tlen[3] = su.T + 1
    rejected("window length", tlen_d=torch.from_numpy(tlen).to(device))
    rc, again = su.call(1, "ledoit_wolf")        # the library still works
    assert rc == 0 and torch.equal(again, good)
    # the engine checks the table against the panel before anything is launched
    pan = engine.Panel(su.R[:40], device=device)
    r_d, t_d = pan.rows_to_device(np.arange(30, 50, dtype=np.int32)[None], np.array([20], dtype=np.int32))
    with pytest.raises(ValueError):
        engine.shrinkage_intensity(pan, r_d, t_d)
    with pytest.raises(ValueError):
        engine.shrinkage_intensity(pan, r_d, t_d, kind="james_stein")


# ---- per-window API -----------------------------------------------------------------------

@pytest.mark.parametrize("method", sm.KINDS)
@pytest.mark.parametrize("n", [24, 130])
def test_covariance_estimate_per_window(device, method, n):
    R = _panel(130)[200:260, :n]
    X = pd.DataFrame(R, columns=[f"a{i}" for i in range(n)])
    cov = Covariance(method=method)
    assert cov.shrinkage_ is None
    S = cov.estimate(X)
    ref, delta = sm.shrunk_cov(R, method)
    assert isinstance(S, pd.DataFrame) and list(S.index) == list(X.columns) and list(S.columns) == list(X.columns)
    assert isinstance(cov.shrinkage_, float) and abs(sm.LD(cov.shrinkage_) - delta) <= 1e-12
    assert 0.0 < cov.shrinkage_ < 1.0
    assert np.abs(sm.LD(1) * S.to_numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    fn = cov_ledoit_wolf if method == "ledoit_wolf" else cov_oas
    assert np.array_equal(fn(X).to_numpy(), S.to_numpy())
    assert isinstance(fn(R), np.ndarray)
    Xn = X.copy()
    Xn.iloc[17, 3] = np.nan
    with pytest.raises(ValueError, match=f"{method} shrinkage needs complete windows"):
        cov.estimate(Xn)


# ---- Backtest.run ----------------------------------------------------------------------------

def _service(opt, X, y, rebdates, box_kw, width=252):
    return BacktestService(
        data={"return_series": X, "bm_series": y},
        selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
        optimization_item_builders={
            "return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
            "bm_series": OptimizationItemBuilder(bibfn=bibfn_bm_series, width=width),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=1),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, **box_kw)},
        optimization=opt, rebdates=rebdates, quiet=True)


def _synthetic(n, D, seed):
    dates, R, y, _ = factor_panel(D, n, seed=seed)
    idx = pd.DatetimeIndex(dates)
    return (pd.DataFrame(R, index=idx, columns=[f"a{i}" for i in range(n)]),
            pd.DataFrame({"bm": y}, index=idx))


def _mv(method):
    return MeanVariance(covariance=Covariance(method=method), solver_name="mi355x", risk_aversion=2.0)


@pytest.mark.parametrize("method", sm.KINDS)
@pytest.mark.parametrize("n,ndates,path", [(300, 24, "lowrank"), (24, 12, "dense")])
def test_backtest_matches_oracle(device, method, n, ndates, path):
    """Backtest.run with a shrinkage covariance on the window route (n = 300 > width = 60) and
    the dense route (n = 24): every date solved, per-date intensities equal to the model's and
    not shared, weights and objective of three dates against the oracle IPM on
    P = 2 ra Sigma*_model (the bounds of test_backtest_lowrank_path_matches_oracle)."""
    from oracle.qp_ipm import solve_qp
    width, ra = 60, 2.0
    X, y = _synthetic(n, 160, seed=11)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + ndates]]
    opt = _mv(method)
    bt = Backtest()
    bt.run(_service(opt, X, y, rebdates, {"upper": 0.1}, width=width))
    assert bt.stats["solved"] == len(rebdates) and bt.stats["path"] == path
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    Xv = X.to_numpy()
    ends = [X.index.get_loc(pd.Timestamp(d)) for d in rebdates]
    delta = opt.covariance.shrinkage_batch_.cpu().numpy()
    model = np.array([float(sm.stats(Xv[e - width + 1:e + 1], method)[3]) for e in ends])
    assert delta.shape == (ndates,) and np.abs(delta - model).max() <= 1e-12
    assert np.diff(np.sort(model)).min() > 1e-9                          # per date, not shared
    for i in (0, 11, ndates - 1):
        Xw = Xv[ends[i] - width + 1:ends[i] + 1]
        P = 2 * ra * np.asarray(sm.shrunk_cov(Xw, method)[0], dtype=np.float64)
        q = -rp.mean_geometric(Xw, None, None, None)
        o = solve_qp(P, q, A=np.ones((1, n)), b=np.ones(1), lb=np.zeros(n), ub=np.full(n, 0.1))
        obj = 0.5 * W[i] @ P @ W[i] + q @ W[i]
        assert abs(obj - o.obj) <= 1e-6 * max(abs(o.obj), 1e-12), (method, i, obj, o.obj)
        assert np.abs(W[i] - o.x).max() < 1e-5, (method, i, np.abs(W[i] - o.x).max())
        assert abs(W[i].sum() - 1) < 1e-7 and W[i].min() > -1e-7 and W[i].max() < 0.1 + 1e-7


@pytest.mark.parametrize("method", sm.KINDS)
def test_backtest_serial_equals_batched(device, method):
    """settings['batched'] = False (Covariance.estimate per date) against the batched run, to
    the bound of tests/test_api_gpu.py::test_backtest_serial_equals_batched."""
    width = 60
    X, y = _synthetic(24, 160, seed=11)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + 12]]
    W = []
    for batched in (True, False):
        bs = _service(_mv(method), X, y, rebdates, {"upper": 0.1}, width=width)
        bs.settings["batched"] = batched
        bt = Backtest()
        bt.run(bs)
        W.append(bt.strategy.get_weights_df().to_numpy(dtype=float))
    assert np.abs(W[0] - W[1]).max() < 1e-7


def test_estimate_batch_lr_contract(device):
    """The 4-tuple keeps the raw S / dg, p_diag = delta mean(diag S), delta in shrinkage_batch_
    (None after any other method), windows with NaN are not batchable."""
    pan = engine.Panel(_panel(64)[:80], device=device)
    rows, tlen = pan.rows_to_device(np.arange(40, dtype=np.int32)[None] + np.arange(3, dtype=np.int32)[:, None],
                                    np.full(3, 40, dtype=np.int32))
    cov = Covariance(method="oas")
    for mat in (True, False):
        S, pdiag, mu, dg = cov.estimate_batch_lr(pan, rows, tlen, materialise=mat)
        d = cov.shrinkage_batch_
        assert d.shape == (3,) and (S is None) == (not mat)
        for b in range(3):
            Sm, dm = sm.shrunk_cov(_panel(64)[b:b + 40], "oas")
            md = np.trace(np.cov(_panel(64)[b:b + 40], rowvar=False)) / 64
            assert abs(d[b].item() - float(dm)) <= 1e-12
            assert abs(pdiag[b].item() - float(dm) * md) <= 1e-12 * md
    cov.spec["method"] = "linear_shrinkage"
    cov.estimate_batch_lr(pan, rows, tlen)
    assert cov.shrinkage_batch_ is None
    nanpan = engine.Panel(np.where(np.arange(80 * 64).reshape(80, 64) == 777, np.nan, _panel(64)[:80]), device=device)
    cov.spec["method"] = "oas"
    assert cov.estimate_batch_lr(nanpan, rows, tlen) == (None, None, None, None)


# ---- workload hook ------------------------------------------------------------------------

def test_workload_hook(device):
    """MinVarianceBacktest(n=130, T=33, D=40, shrinkage='ledoit_wolf') (delta ~ 0.45): one step
    solves every date on the per-date band route with the model's ridge, certified against
    P = 2 (1 - delta) S + p_diag I recomputed from the panel rows."""
    wl = MinVarianceBacktest(n=130, T=33, D=40, shrinkage="ledoit_wolf", device=device)
    assert wl.use_lr
    res = wl.step()
    torch.cuda.synchronize()
    assert np.all(res.status.cpu().numpy() == _lib.PQ_SOLVED)
    assert res.capacitance == "band"            # per-date values: no shared group capacitance
    c = wl.certificate(res)
    assert c["max_violation"] <= 1e-7, c
    assert c["max_rel_stationarity"] <= 1e-7, c  # the bound of tests/test_headline_parity_gpu.py
    pd_gpu = wl.qb.p_diag.cpu().numpy()
    ws_gpu = wl.w_scale.cpu().numpy()
    for d in range(wl.D):
        e = wl.ends_local[d]
        Xw = wl.R_rank[e - wl.T + 1:e + 1]
        a, f, g, delta = sm.stats(Xw, "ledoit_wolf")
        want = 2 * delta * a / (sm.LD(wl.n) * (wl.T - 1))
        assert abs(sm.LD(pd_gpu[d]) - want) <= 1e-12 * want, (d, pd_gpu[d], float(want))
        assert abs(sm.LD(ws_gpu[d]) - (1 - delta) / (wl.T - 1)) <= 1e-12
        assert 0.0 < delta < 1.0                 # the model's: not clipped
    assert len(np.unique(pd_gpu)) == wl.D
    with pytest.raises(ValueError):
        MinVarianceBacktest(n=130, T=33, D=4, shrinkage="james_stein", device=device)


def test_workload_without_shrinkage_is_unchanged(device):
    """shrinkage=None (the default, what bench.py builds): no ridge, no shrinkage stage, and
    the weights are bit-equal to those of a default-constructed twin, step by step."""
    wl = MinVarianceBacktest(n=130, T=33, D=40, shrinkage=None, device=device)
    twin = MinVarianceBacktest(n=130, T=33, D=40, device=device)
    assert wl.qb.p_diag is None and twin.qb.p_diag is None and twin.shrinkage is None
    ev = []
    for k in range(2):   # first and second step of each object
        x1 = wl.step(events=ev).x.clone()
        x2 = twin.step().x.clone()
        torch.cuda.synchronize()
        assert torch.equal(x1, x2), k
    assert "shrinkage" not in [e[0] for e in ev]
    ws = 1.0 / (wl.tlen_d.to(F64) - 1.0)
    assert torch.equal(wl.w_scale, ws)
