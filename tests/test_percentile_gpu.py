"""Quantile portfolios on the device: pq_percentile_batched / engine.percentile_weights,
PercentilePortfolios.solve and the batched Backtest.run against the numpy restatement of the
reference loop (tests/percentile_model.py) and the fixture captured from the reference itself
(tests/golden/msci_percentile.npz, tools/capture_percentile.py).

Everything here is exact: thresholds, bucket ids, counts, weights and status are compared
with ``==`` on every row, no tolerance.  Thresholds are also compared bit for bit with
np.percentile wherever they are not a zero: which of -0.0 / +0.0 sits at an order statistic of
a row that holds both is the sorter's choice (numpy's partition makes one too), and the sign
of a zero decides no comparison."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.backtest import Backtest, BacktestService, append_custom
from porqua_amd.builders import (OptimizationItemBuilder, SelectionItemBuilder, bibfn_box_constraints,
                                 bibfn_bm_series, bibfn_budget_constraint, bibfn_return_series,
                                 bibfn_selection_data)
from porqua_amd.helper_functions import output_to_strategies
from porqua_amd.mean_estimation import MeanEstimator
from porqua_amd.optimization import Objective, PercentilePortfolios
from tests.conftest import load_golden
from tests.percentile_model import PCT_EMPTY_BUCKET, PCT_NAN_SCORE, PCT_OK, batch_model, reference_solve

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _mixed_rows(n, B, rng):
    cont = rng.standard_normal(n)
    tied = np.round(rng.standard_normal(n), 1)             # ties straddle the thresholds
    ints = rng.integers(-3, 4, n).astype(np.float64)
    ints[ints == 0] *= rng.choice([-1.0, 1.0], int((ints == 0).sum()))   # both zeros
    flat = np.full(n, 0.25)                                # all equal: empty buckets for N >= 2
    nan = rng.standard_normal(n)
    nan[int(rng.integers(n))] = np.nan
    rets = 0.01 * rng.standard_normal(n)                   # return-like, next to the failing rows
    if B == 3:
        return np.array([tied, nan, cont])
    return np.array([cont, tied, flat, ints, nan, rets, np.round(rets, 3)])


@pytest.mark.parametrize("N", [1, 2, 5, 10])
@pytest.mark.parametrize("n", [1, 5, 11, 63, 64, 65, 101, 1000, 1025, 8193, 16384])
def test_kernel_equals_the_restatement(device, n, N):
    B = 7 if n < 8000 else 3
    rng = np.random.default_rng(1000 * n + N)
    X = _mixed_rows(n, B, rng)
    ld = n + 3
    Xp = np.full((B, ld), np.nan)                          # padding columns must never be read
    Xp[:, :n] = X
    th_m, bucket_m, counts_m, w_m, status_m = batch_model(X, N)
    w, bucket, counts, th, status = engine.percentile_weights(torch.from_numpy(Xp).to(device), N, n=n)
    th, w = th.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(status.cpu().numpy(), status_m)
    assert np.array_equal(bucket.cpu().numpy(), bucket_m)
    assert np.array_equal(counts.cpu().numpy(), counts_m)
    assert np.array_equal(w, w_m, equal_nan=True)
    assert np.array_equal(th, th_m, equal_nan=True)        # th_m is np.percentile itself
    nz = np.isfinite(th_m) & (th_m != 0)
    assert np.array_equal(_bits(th)[nz], _bits(th_m)[nz])
    # the failing rows are the ones the restatement fails on, and only those
    nan_row = 1 if B == 3 else 4
    assert status_m[nan_row] == PCT_NAN_SCORE and np.isnan(w[nan_row]).all()
    if B == 7:
        assert status_m[2] == (PCT_EMPTY_BUCKET if N >= 2 else PCT_OK)
    if N > n:
        assert np.all(status_m[np.arange(B) != nan_row] == PCT_EMPTY_BUCKET)
    ok = status_m == PCT_OK
    assert np.isfinite(w[ok]).all()


def test_gamma_zero_thresholds_sit_on_scores(device):
    """n = 101 with N = 5 and n = 11 with N = 10: every threshold is an order statistic, so a
    score equals its threshold and ``<=`` decides its bucket."""
    for n, N in ((101, 5), (11, 10)):
        assert np.all(engine.percentile_plan(n, N)[2][:-1] == 0)
        x = np.random.default_rng(n).permutation(n).astype(np.float64)[None]
        w, bucket, counts, th, status = engine.percentile_weights(torch.from_numpy(x).to(device), N, sign=1.0)
        assert np.array_equal(th[0].cpu().numpy(), np.arange(N + 1) * ((n - 1) // N))
        assert np.array_equal(bucket.cpu().numpy(), batch_model(x, N, sign=1.0)[1])
        assert counts[0, 0].item() == (n - 1) // N + 1 and status[0].item() == PCT_OK


def test_limits_raise_value_error(device):
    x = torch.zeros((1, 16385), dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match="16384"):
        engine.percentile_weights(x, 5)
    with pytest.raises(ValueError, match="256"):
        engine.percentile_weights(x[:, :100], 257)
    # the C entry refuses the same shapes itself, naming the limit
    lib = _lib.load()
    p = ctypes.c_void_p(x.data_ptr())
    for n, N, limit in ((16385, 5, b"16384"), (100, 257, b"256")):
        rc = lib.pq_percentile_batched(p, 16385, n, 1, -1.0, N, p, p, p, p, p, p, p, p, engine._stream())
        assert rc != 0 and limit in lib.pq_last_error()


# ---- PercentilePortfolios.solve ------------------------------------------------------------


def _names():
    return [str(c) for c in load_golden("msci_panel")["columns"]]


@pytest.mark.parametrize("N", [1, 3, 5])
def test_solve_reproduces_the_reference_fixture(device, N):
    g, names = load_golden("msci_percentile"), _names()
    for s, w_ref, masks in zip(g["a_scores"], g[f"a_w_{N}"], g[f"a_masks_{N}"]):
        opt = PercentilePortfolios(n_percentiles=N)
        opt.objective = Objective(scores=-pd.Series(s, index=names))
        assert opt.solve() is True
        assert isinstance(opt.results["weights"], dict) and list(opt.results["weights"]) == names
        assert np.array_equal(np.array([opt.results["weights"][k] for k in names]), w_ref)
        assert list(opt.results["w_dict"]) == list(range(1, N + 1))
        for i in range(1, N + 1):
            ser = opt.results["w_dict"][i]
            assert isinstance(ser, pd.Series)
            assert list(ser.index) == [k for k, m in zip(names, masks[i - 1]) if m]   # universe order
            assert np.all(ser.values == 1 / masks[i - 1].sum())


def test_solve_through_the_estimator_on_a_fixture_window(device):
    """set_objective with the device MeanEstimator on the fixture's windows: the scores differ
    from pandas' in the last bits only (the fixture's threshold-score gap is >= 1e-9), so the
    memberships are the reference's."""
    g, p, names = load_golden("msci_percentile"), load_golden("msci_panel"), _names()
    X = pd.DataFrame(p["returns"], index=pd.DatetimeIndex(p["dates"].astype("datetime64[D]")), columns=names)
    assert float(g["a_gap"].min()) >= 1e-9
    me = MeanEstimator(method="geometric", n_mom=int(g["n_mom"]), n_rev=int(g["n_rev"]))
    for d, s, w_ref in zip(g["a_dates"][:3], g["a_scores"], g["a_w_5"]):
        win = X[X.index <= str(d)].tail(int(g["width"]))
        opt = PercentilePortfolios(estimator=me)
        assert opt.params == {"solver_name": "percentile", "n_percentiles": 5, "field": None}
        opt.set_objective({"return_series": win[win.index.dayofweek < 5]})
        assert np.abs(-opt.objective["scores"].to_numpy() / s - 1).max() < 1e-12
        opt.solve()
        assert np.array_equal(np.array([opt.results["weights"][k] for k in names]), w_ref)


def test_solve_raises_zero_division_on_equal_scores(device):
    opt = PercentilePortfolios(n_percentiles=3)
    opt.objective = Objective(scores=-pd.Series(np.full(12, 0.5), index=list("abcdefghijkl")))
    with pytest.raises(ZeroDivisionError):
        opt.solve()
    opt.objective = Objective(scores=-pd.Series([0.1, np.nan, 0.3, 0.2], index=list("abcd")))
    with pytest.raises(ZeroDivisionError):
        opt.solve()


def test_field_and_score_weight_forms(device):
    rng = np.random.default_rng(5)
    idx = [f"A{i}" for i in range(13)]
    scores = pd.DataFrame({"f1": rng.standard_normal(13), "f2": np.round(rng.standard_normal(13), 1)}, index=idx)
    data = {"scores": scores}
    sw = {"f1": 0.25, "f2": 0.75}
    forms = [(dict(field="f1"), None, scores["f1"]),
             (dict(), sw, scores[sw.keys()].multiply(sw.values()).sum(axis=1)),
             (dict(), None, scores.mean(axis=1).squeeze())]
    for kw, score_weights, expect in forms:
        opt = PercentilePortfolios(n_percentiles=4, **kw)
        if score_weights is not None:   # params is rebuilt by __init__, as in the reference
            opt.params["score_weights"] = score_weights
        opt.set_objective(data)
        assert np.array_equal(opt.objective["scores"].to_numpy(), -expect.to_numpy())
        opt.solve()
        _, masks, w = reference_solve(-expect.to_numpy(), 4)
        assert np.array_equal(np.array([opt.results["weights"][k] for k in idx]), w)
        for i in range(4):
            assert list(opt.results["w_dict"][i + 1].index) == [k for k, m in zip(idx, masks[i]) if m]
    both = PercentilePortfolios(field="f1", estimator=MeanEstimator())
    with pytest.raises(ValueError, match="not both"):
        both.set_objective(data)


# ---- batched Backtest.run ------------------------------------------------------------------


def _service(X, rebdates, width, optimization, bm=None, **settings):
    opt_builders = {"return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
                    "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=1),
                    "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, upper=0.1)}
    data = {"return_series": X}
    if bm is not None:
        data["bm_series"] = bm
        opt_builders["bm_series"] = OptimizationItemBuilder(bibfn=bibfn_bm_series, width=width)
    return BacktestService(data=data,
                           selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
                           optimization_item_builders=opt_builders, optimization=optimization,
                           rebdates=list(rebdates), quiet=True, **settings)


def test_batched_backtest_reproduces_the_reference_walkthrough(device):
    g, p, names = load_golden("msci_percentile"), load_golden("msci_panel"), _names()
    idx = pd.DatetimeIndex(p["dates"].astype("datetime64[D]"))
    X = pd.DataFrame(p["returns"], index=idx, columns=names)
    bm = pd.DataFrame({"bm": p["bm"]}, index=idx)
    rebdates = [str(d) for d in g["b_all_rebdates"]]
    me = MeanEstimator(method="geometric", scalefactor=1, n_mom=int(g["n_mom"]), n_rev=int(g["n_rev"]))
    opt = PercentilePortfolios(n_percentile=5, estimator=me)      # (sic) the walkthrough's ignored keyword
    bs = _service(X, rebdates, int(g["width"]), opt, bm=bm, append_fun=append_custom, append_fun_args=["w_dict"])
    bt = Backtest()
    bt.run(bs)
    assert bt.stats["path"] == "percentile"
    assert bt.stats["bucket"].shape == (len(rebdates), 24) and bt.stats["counts"].shape == (len(rebdates), 5)
    assert [pf.rebalancing_date for pf in bt.strategy.portfolios] == rebdates
    assert float(g["b_gap"].min()) >= 1e-9
    for d, w_ref, masks in zip(g["b_rebdates"], g["b_w"], g["b_masks"]):
        i = rebdates.index(str(d))
        assert np.array_equal(bt.stats["bucket"][i][None] == np.arange(1, 6)[:, None], masks)
        assert np.array_equal(np.array([bt.strategy.portfolios[i].weights[k] for k in names]), w_ref)
        for q in range(1, 6):
            ser = bt.output[str(d)][f"weights_{q}"]
            members = [k for k, m in zip(names, masks[q - 1]) if m]
            assert list(ser.index) == members and np.all(ser.values == 1 / len(members))
    strategies = output_to_strategies(bt.output)
    assert list(strategies) == ["q1", "q2", "q3", "q4", "q5"]
    for s in strategies.values():
        r = s.simulate(return_series=X, fc=0, vc=0)
        assert len(r) > 3000 and np.isfinite(r.to_numpy()).all()
    # without an append_fun the portfolios are lazy rows of the same weight panel
    bs2 = _service(X, rebdates, int(g["width"]), PercentilePortfolios(estimator=me), bm=bm)
    bt2 = Backtest()
    bt2.run(bs2)
    assert bt2.stats["path"] == "percentile" and not bt2.output
    assert all(a.weights == b.weights for a, b in zip(bt.strategy.portfolios, bt2.strategy.portfolios))
    assert bs2.optimization.results["weights"] == bt.strategy.portfolios[-1].weights


def _gap(x, N):
    """Smallest relative distance between a threshold strictly between two scores and a score."""
    v = (len(x) - 1) * (np.linspace(0, 100, N + 1) / 100)
    th = np.percentile(x, np.linspace(0, 100, N + 1))
    return min(float(np.min(np.abs(th[t] - x) / np.maximum(np.abs(th[t]), np.abs(x))))
               for t in np.flatnonzero(v != np.floor(v)))


@pytest.mark.parametrize("first,spec", [
    (100, dict(n_mom=126, n_rev=21)),   # windows of 101 .. 140 rows, all short of 252 and ragged; the
                                        # estimator's sub-window start moves once a window passes 126 rows
    (260, dict())])                     # full 252-row windows, the whole window scored (sliding groups)
def test_batched_equals_serial(device, first, spec):
    rng = np.random.default_rng(11)
    n, D = 494, first + 50
    idx = pd.bdate_range("2015-01-01", periods=D)
    names = [f"S{i:03d}" for i in range(n)]
    X = pd.DataFrame(0.01 * rng.standard_normal((D, n)), index=idx, columns=names)
    rebdates = [str(d.date()) for d in idx[first:first + 40]]
    me = MeanEstimator(method="geometric", **spec)
    seen = {}

    def keep(backtest, bs, rebalancing_date, what):
        seen[rebalancing_date] = bs.optimization.objective["scores"].to_numpy().copy()
        append_custom(backtest=backtest, bs=bs, rebalancing_date=rebalancing_date, what=what)

    serial = Backtest()
    serial.run(_service(X, rebdates, 252, PercentilePortfolios(estimator=me), batched=False,
                        append_fun=keep, append_fun_args=["w_dict"]))
    assert serial.stats.get("path") != "percentile" and len(seen) == 40
    # the two paths compute the scores with the same kernel over different row tables; a
    # rounding difference could decide a membership only if a score sat on a threshold
    assert min(_gap(x, 5) for x in seen.values()) >= 1e-9
    batched = Backtest()
    batched.run(_service(X, rebdates, 252, PercentilePortfolios(estimator=me),
                         append_fun=append_custom, append_fun_args=["w_dict"]))
    assert batched.stats["path"] == "percentile"
    for a, b in zip(serial.strategy.portfolios, batched.strategy.portfolios):
        assert a.rebalancing_date == b.rebalancing_date and a.weights == b.weights
    for d in rebdates:
        for q in range(1, 6):
            sa, sb = serial.output[d][f"weights_{q}"], batched.output[d][f"weights_{q}"]
            assert list(sa.index) == list(sb.index) and np.array_equal(sa.values, sb.values)


def test_backtest_raises_runtime_error_naming_the_date(device):
    """A date whose scores all tie (a window of zero returns) has empty buckets: the batched
    run raises RuntimeError naming it, as the serial rebalance() does for ZeroDivisionError."""
    rng = np.random.default_rng(2)
    idx = pd.bdate_range("2018-01-01", periods=80)
    R = 0.01 * rng.standard_normal((80, 20))
    R[20:50] = 0.0
    X = pd.DataFrame(R, index=idx, columns=[f"S{i}" for i in range(20)])
    rebdates = [str(d.date()) for d in idx[45:60]]         # the window of row 49 is all zeros
    for settings in (dict(), dict(batched=False)):
        bt = Backtest()
        with pytest.raises(RuntimeError, match="division by zero" + ("" if settings else ".*" + rebdates[4])):
            bt.run(_service(X, rebdates, 30, PercentilePortfolios(estimator=MeanEstimator()), **settings))


def test_at_size_from_device_geometric_means(device):
    rng = np.random.default_rng(3)
    n, B, width, N = 1000, 256, 252, 5
    D = width + B
    dates = pd.bdate_range("2012-01-02", periods=D).values.astype("datetime64[D]")
    panel = engine.Panel(0.01 * rng.standard_normal((D, n)), device=device)
    rows, tlen = engine.window_rows(dates, dates[width:], width)
    mu = panel.window_means(*panel.rows_to_device(rows, tlen), geometric=True)
    w, bucket, counts, th, status = engine.percentile_weights(mu, N, n=n)
    th_m, bucket_m, counts_m, w_m, status_m = batch_model(mu[:, :n].cpu().numpy(), N)
    assert np.all(status_m == PCT_OK) and np.array_equal(status.cpu().numpy(), status_m)
    assert np.array_equal(bucket.cpu().numpy(), bucket_m)
    assert np.array_equal(w.cpu().numpy(), w_m)
    assert np.array_equal(counts.cpu().numpy(), counts_m) and np.array_equal(th.cpu().numpy(), th_m)
