"""l1 row: transaction cost / turnover budget around x0.

Golden problems were captured from the reference's own Backtest.run + model_qpsolvers
(tools/capture_l1.py -> tests/golden/msci_l1_{tc,to}.npz: the 2n-variable linearised
problems of src/qp_problems.py:40-77, 120-157, with KKT-certified oracle optima).

* CPU: the package's linearisation reproduces the captured matrices; the signed split
  (porqua_amd/l1split.py) solved by the oracle IPM gives the golden weights / objective.
* GPU: QuadraticProgram(solver 'mi355x') with the linearisation solves the split on the
  device.  Bars: weights 1e-5 (L-inf), objective 1e-6 relative, violation 1e-7.
"""
import os

import numpy as np
import pytest

from oracle.qp_ipm import solve_qp
from porqua_amd.l1split import L1Split, merge_solution, split_problem
from porqua_amd.qp_problems import QuadraticProgram

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = {"tc": "cost", "to": "budget", "lev": "budget"}
TAGS = ["tc", "to", "lev"]


def _case(tag, i):
    g = np.load(os.path.join(GOLD, f"msci_l1_{tag}.npz"))
    n = g["P"].shape[-1] // (3 if tag == "lev" else 2)
    b0 = np.atleast_1d(g["b"][i])[:1]
    base = dict(P=g["P"][i][:n, :n], q=g["q"][i][:n], A=g["A"][i][:1, :n], b=b0,
                lb=g["lb"][i][:n], ub=g["ub"][i][:n], G=None, h=None)
    value = 0.002 if tag == "tc" else float(g["h"][i][-1])
    if tag == "lev":
        return g, n, base, L1Split("budget", np.zeros(n), value, layout="pm")
    return g, n, base, L1Split(KINDS[tag], g["x0"], value)


def _qp(base, term, solver):
    qp = QuadraticProgram(P=base["P"].copy(), q=base["q"].copy(), A=base["A"].copy(), b=base["b"].copy(),
                          lb=base["lb"].copy(), ub=base["ub"].copy(), G=None, h=None,
                          params={"solver_name": solver})
    if term.layout == "pm":
        qp.linearize_leverage_constraint(N=term.x0.size, leverage_budget=term.value)
    elif term.kind == "cost":
        qp.linearize_turnover_objective(term.x0, transaction_cost=term.value)
    else:
        qp.linearize_turnover_constraint(term.x0, to_budget=term.value)
    return qp


@pytest.mark.parametrize("tag", TAGS)
def test_linearisation_matches_reference(tag):
    for i in (0, 7, 23):
        g, n, base, term = _case(tag, i)
        qp = _qp(base, term, "mi355x")
        # the captured P went through the reference's PD repair (src/qp_problems.py:189-191),
        # which adds ~1e-19 to the zero auxiliary block
        assert np.allclose(qp["P"], g["P"][i], rtol=0, atol=1e-15 * np.abs(g["P"][i]).max())
        for k in ("q", "G", "h", "lb", "ub"):
            assert np.array_equal(np.asarray(qp[k], dtype=float).reshape(g[k][i].shape), g[k][i]), k
        assert np.array_equal(qp["A"].reshape(g["A"][i].shape), g["A"][i])
        # leverage: the reference leaves b 0-d (a defect, see tools/capture_l1.py); the
        # fixture and this package hold the intended [b; 0]
        assert np.array_equal(np.asarray(qp["b"], dtype=float).reshape(-1), np.atleast_1d(g["b"][i]))


@pytest.mark.parametrize("tag", TAGS)
def test_split_solved_by_oracle_matches_golden(tag):
    for i in range(0, 24, 3):
        g, n, base, term = _case(tag, i)
        sp = split_problem(base, term)
        s = solve_qp(sp["P"], sp["q"], sp["G"], sp["h"], sp["A"], sp["b"], sp["lb"], sp["ub"])
        x, d = merge_solution(s.x, term)
        assert np.abs(x - g["x"][i][:n]).max() < 1e-6
        obj_ref = 0.5 * g["x"][i] @ g["P"][i] @ g["x"][i] + g["q"][i] @ g["x"][i]
        obj = 0.5 * x @ base["P"] @ x + base["q"] @ x + (term.value * d.sum() if term.kind == "cost" else 0.0)
        assert abs(obj - obj_ref) <= 1e-8 * max(1.0, abs(obj_ref))


def test_merged_vector_satisfies_linearised_rows():
    """merge_solution's full vector [x; aux] satisfies the reference's linearised equality
    rows (leverage: x + x+ - x- = 0, src/qp_problems.py:79-118) and the turnover rows
    (d >= |x - x0|)."""
    for tag in TAGS:
        g, n, base, term = _case(tag, 3)
        qp = _qp(base, term, "mi355x")
        sp = split_problem(base, term)
        s = solve_qp(sp["P"], sp["q"], sp["G"], sp["h"], sp["A"], sp["b"], sp["lb"], sp["ub"])
        x, aux = merge_solution(s.x, term)
        full = np.concatenate([x, aux])
        A = np.atleast_2d(qp["A"])
        assert np.abs(A @ full - np.asarray(qp["b"], dtype=float).reshape(-1)).max() < 1e-9, tag
        if qp.get("G") is not None:
            assert (np.atleast_2d(qp["G"]) @ full - np.asarray(qp["h"]).reshape(-1)).max() < 1e-9, tag


def test_zero_transaction_cost_keeps_the_turnover_budget():
    """transaction_cost = 0 with a turnover constraint: the reference applies both
    linearisations (src/optimization.py:131-137: 0 is not None, and `not 0`), so the
    budget binds; the batched backtest's term must be the budget, not a zero cost."""
    from porqua_amd.l1split import term_from_model

    class C:
        l1 = {"turnover": {"x0": {"a": 0.5, "b": 0.5}, "rhs": 0.3}}

    t = term_from_model(C(), {"transaction_cost": 0.0}, ["a", "b", "c"])
    assert t.kind == "budget" and t.value == 0.3 and np.array_equal(t.x0, [0.5, 0.5, 0.0])
    t = term_from_model(C(), {"transaction_cost": 0.01}, ["a", "b", "c"])
    assert t.kind == "cost" and t.value == 0.01
    t = term_from_model(C(), {}, ["a", "b", "c"])
    assert t.kind == "budget"


def test_split_rejects_x0_outside_box():
    g, n, base, term = _case("tc", 0)
    bad = L1Split("cost", np.full(n, 2.0), 0.002)
    with pytest.raises(NotImplementedError):
        split_problem(base, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_device_l1_matches_golden(tag):
    for i in range(24):
        g, n, base, term = _case(tag, i)
        qp = _qp(base, term, "mi355x")
        qp.solve()
        s = qp["solution"]
        assert s.found and s.extras.get("l1_split") == term.kind
        x = s.x[:n]
        assert np.abs(x - g["x"][i][:n]).max() < 1e-5, (i, np.abs(x - g["x"][i][:n]).max())
        obj_ref = float(g["obj"][i])
        assert abs(s.obj - obj_ref) <= 1e-6 * max(1.0, abs(obj_ref))
        viol = max(abs(x.sum() - 1.0), float(np.maximum(base["lb"] - x, 0).max()),
                   float(np.maximum(x - base["ub"], 0).max()),
                   (np.abs(x - term.x0).sum() - term.value) if term.kind == "budget" else 0.0)
        assert viol <= 1e-7


def _msci():
    import pandas as pd
    p = np.load(os.path.join(GOLD, "msci_panel.npz"))
    idx = pd.DatetimeIndex(p["dates"].astype("datetime64[D]"))
    cols = [str(c) for c in p["columns"]]
    return pd.DataFrame(p["returns"], index=idx, columns=cols), pd.DataFrame({"bm": p["bm"]}, index=idx)


def _service(opt, X, y, rebdates, extra=None, width=252, box_kw=None):
    from porqua_amd.backtest import BacktestService
    from porqua_amd.builders import (OptimizationItemBuilder, SelectionItemBuilder, bibfn_bm_series,
                                     bibfn_box_constraints, bibfn_budget_constraint, bibfn_return_series,
                                     bibfn_selection_data)
    blds = {"return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
            "bm_series": OptimizationItemBuilder(bibfn=bibfn_bm_series, width=width),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=1),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, **(box_kw or {}))}
    if extra is not None:
        blds["l1"] = extra
    return BacktestService(data={"return_series": X, "bm_series": y},
                           selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
                           optimization_item_builders=blds, optimization=opt, rebdates=rebdates, quiet=True)


@pytest.mark.gpu
def test_device_backtest_transaction_cost_matches_reference():
    """The reference's own msci backtest with transaction_cost around params['x0']
    (tools/capture_l1.py), batched on the device through the split."""
    from porqua_amd.backtest import Backtest
    from porqua_amd.covariance import Covariance
    from porqua_amd.optimization import MeanVariance
    g = np.load(os.path.join(GOLD, "msci_l1_tc.npz"))
    X, y = _msci()
    n = X.shape[1]
    x0 = dict(zip(X.columns, g["x0"]))
    opt = MeanVariance(covariance=Covariance(method="linear_shrinkage", lambda_covmat_regularization=0.1),
                       solver_name="mi355x", transaction_cost=0.002, x0=x0)
    bt = Backtest()
    bt.run(_service(opt, X, y, [str(d) for d in g["rebdates"]]))
    assert bt.stats["solved"] == len(g["rebdates"])         # batched path, all solved
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    assert np.abs(W - g["x"][:, :n]).max() < 1e-5
    obj = bt.stats["objective"]
    assert np.max(np.abs(obj - g["obj"]) / np.maximum(np.abs(g["obj"]), 1e-12)) < 1e-6


@pytest.mark.gpu
def test_device_backtest_turnover_budget_matches_reference():
    """A custom l1 builder (serial loop, one split QP per date) against the reference."""
    from porqua_amd.backtest import Backtest
    from porqua_amd.builders import OptimizationItemBuilder
    from porqua_amd.optimization import LeastSquares
    g = np.load(os.path.join(GOLD, "msci_l1_to.npz"))
    X, y = _msci()
    n = X.shape[1]
    x0 = dict(zip(X.columns, g["x0"]))

    def add_turnover(bs, rebdate, **kw):
        bs.optimization.constraints.add_l1("turnover", rhs=kw["rhs"], x0=kw["x0"])

    opt = LeastSquares(l2_penalty=1e-3, solver_name="mi355x")
    bt = Backtest()
    bt.run(_service(opt, X, y, [str(d) for d in g["rebdates"]],
                    extra=OptimizationItemBuilder(bibfn=add_turnover, rhs=0.3, x0=x0)))
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    assert np.abs(W - g["x"][:, :n]).max() < 1e-5
    assert np.all(np.abs(W - g["x0"][None, :]).sum(1) <= 0.3 + 1e-7)


def _sparse_w0(n, ub=0.1):
    """A long-only previous portfolio that sits at its bounds: about 80 % of the weights exactly 0
    (= lb) and two exactly at ub; the rest positive below ub, summing to 1."""
    rng = np.random.default_rng(9)
    w0 = np.zeros(n)
    held = rng.choice(n, size=n // 5, replace=False)
    w0[held[:2]] = ub
    w = rng.uniform(0.2, 1.0, size=held.size - 2)
    w0[held[2:]] = (1.0 - 2 * ub) * w / w.sum()
    assert (w0 == 0).mean() >= 0.79 and (w0 == ub).sum() == 2 and w0.max() <= ub and abs(w0.sum() - 1) < 1e-12
    return w0


def _window_path_l1(shrink, w0, kind, value):
    """n > window: the split runs on the Woodbury (window) path with the panel [R, -R];
    checked against the oracle IPM on the split problem per date.  ``kind`` 'cost': a
    transaction cost ``value`` around w0; 'budget': the turnover budget sum|x - w0| <= value."""
    import pandas as pd
    from porqua_amd.backtest import Backtest
    from porqua_amd.builders import OptimizationItemBuilder
    from porqua_amd.covariance import Covariance
    from porqua_amd.optimization import MeanVariance
    from porqua_amd.synthetic import factor_panel
    from oracle import ref_pipeline as rp
    n, D, width = 200, 120, 60
    dates, R, yv, _ = factor_panel(D, n, seed=3)
    idx = pd.DatetimeIndex(dates)
    X = pd.DataFrame(R, index=idx, columns=[f"a{i}" for i in range(n)])
    y = pd.DataFrame({"bm": yv}, index=idx)
    rebdates = [str(d.date()) for d in X.index[width + 2:width + 2 + 16]]
    cov = Covariance(method="linear_shrinkage", lambda_covmat_regularization=0.1) if shrink else Covariance()
    x0 = dict(zip(X.columns, w0))
    if kind == "cost":
        opt = MeanVariance(covariance=cov, solver_name="mi355x", transaction_cost=value, x0=x0)
        bs = _service(opt, X, y, rebdates, width=width, box_kw={"upper": 0.1})
    else:
        def add_turnover(bs, rebdate, **kw):
            bs.optimization.constraints.add_l1("turnover", rhs=value, x0=x0)

        opt = MeanVariance(covariance=cov, solver_name="mi355x")
        bs = _service(opt, X, y, rebdates, width=width, box_kw={"upper": 0.1},
                      extra=OptimizationItemBuilder(bibfn=add_turnover))
        bs.settings["static_builders"] = True   # the same l1 term every date: the batched path
    bt = Backtest()
    bt.run(bs)
    assert bt.stats["solved"] == len(rebdates) and bt.stats["path"] == "lowrank"
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    tc = value if kind == "cost" else 0.0
    for i in (0, 7, len(rebdates) - 1):
        e = X.index.get_loc(pd.Timestamp(rebdates[i]))
        Xw = R[e - width + 1:e + 1]
        S = rp.cov_pearson(Xw)
        if shrink:
            S = S + 0.1 * np.mean(np.diag(S)) * np.eye(n)
        P, q = 2 * S, -rp.mean_geometric(Xw, None, None, None)
        base = dict(P=P, q=q, A=np.ones((1, n)), b=np.ones(1), G=None, h=None, lb=np.zeros(n),
                    ub=np.full(n, 0.1))
        term = L1Split(kind, w0, value)
        sp = split_problem(base, term)
        o = solve_qp(sp["P"], sp["q"], sp["G"], sp["h"], sp["A"], sp["b"], sp["lb"], sp["ub"])
        xo, do = merge_solution(o.x, term)
        f = lambda x: 0.5 * x @ P @ x + q @ x + tc * np.abs(x - w0).sum()   # noqa: E731
        assert abs(f(W[i]) - f(xo)) <= 1e-6 * max(abs(f(xo)), 1e-12), (i, f(W[i]), f(xo))
        assert abs(bt.stats["objective"][i] - f(W[i])) <= 1e-6 * max(abs(f(xo)), 1e-12)
        if shrink:
            assert np.abs(W[i] - xo).max() < 1e-5
        assert abs(W[i].sum() - 1) < 1e-7 and W[i].min() > -1e-7 and W[i].max() < 0.1 + 1e-7
        if kind == "budget":
            assert np.abs(W[i] - w0).sum() <= value + 1e-7
    return W


@pytest.mark.gpu
@pytest.mark.parametrize("shrink", [True, False])
def test_device_backtest_window_path_transaction_cost(shrink):
    """A Dirichlet previous portfolio: strictly inside the box, so the split box is uniform and the
    band form of the capacitance runs."""
    _window_path_l1(shrink, np.random.default_rng(9).dirichlet(np.ones(200)), "cost", 0.001)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,value", [("cost", 0.001), ("budget", 0.3)])
@pytest.mark.parametrize("shrink", [True, False])
def test_device_backtest_window_path_sparse_previous_portfolio(monkeypatch, shrink, kind, value):
    """The same run from a previous portfolio at its bounds (80 % of the weights exactly 0, two
    exactly at the upper bound 0.1): the split variables of those assets are fixed, [0, 0], next to
    ordinary ones, the box rows no longer share one rho and the solve takes the direct
    capacitance with the unfused grouped ADMM (tests/test_window_mixed_gpu.py) -- the route of
    every long-only backtest with a turnover term and n > T.  Same oracle, same bars; the
    turnover budget additionally holds."""
    from porqua_amd import engine
    seen, solve = [], engine.solve_lowrank

    def spy(*a, **kw):
        res = solve(*a, **kw)
        seen.append(res.capacitance)
        return res

    monkeypatch.setattr(engine, "solve_lowrank", spy)
    w0 = _sparse_w0(200)
    W = _window_path_l1(shrink, w0, kind, value)
    assert seen and all(c == "direct" for c in seen), seen
    assert (np.abs(W - w0[None, :]) > 1e-6).any()   # (it trades)


@pytest.mark.gpu
def test_device_backtest_turnover_and_leverage_together():
    """A turnover budget and a leverage constraint together (two l1 terms: the reference's
    linearised rows, 2n + 2 inequality and n + 1 equality rows).  The serial loop solves each
    date's linearised QP on the device IPM (porqua_amd/ipm.py); with static_builders the
    batched backtest solves all dates at once on the per-asset-block IPM
    (porqua_amd/ipm_l1.py).  Both are checked against the oracle IPM on the captured QPs."""
    from oracle.qp_ipm import solve_qp
    from porqua_amd.backtest import Backtest
    from porqua_amd.builders import OptimizationItemBuilder
    from porqua_amd.covariance import Covariance
    from porqua_amd.optimization import MeanVariance
    X, y = _msci()
    n = X.shape[1]
    rng = np.random.default_rng(9)
    x0 = dict(zip(X.columns, rng.dirichlet(np.ones(n))))

    def add_l1(bs, rebdate, **kw):
        bs.optimization.constraints.add_l1("turnover", rhs=0.4, x0=x0)
        bs.optimization.constraints.add_l1("leverage", rhs=1.3)

    seen = []

    def keep(backtest, bs, rebalancing_date, what):
        m = bs.optimization.model
        seen.append(({k: m.get(k) for k in ("P", "q", "G", "h", "A", "b", "lb", "ub")}, m["solution"]))

    def opt():
        return MeanVariance(covariance=Covariance(method="linear_shrinkage", lambda_covmat_regularization=0.1),
                            solver_name="mi355x", risk_aversion=3.0)
    rebdates = [str(d.date()) for d in X.index[1000:2600:100]]
    box = {"box_type": "LongShort", "lower": -0.1, "upper": 0.3}
    bs = _service(opt(), X, y, rebdates, extra=OptimizationItemBuilder(bibfn=add_l1), box_kw=box)
    bs.settings["append_fun"] = keep
    bt = Backtest()
    bt.run(bs)                                          # custom builder: serial loop
    assert len(seen) == len(rebdates)
    bs2 = _service(opt(), X, y, rebdates, extra=OptimizationItemBuilder(bibfn=add_l1), box_kw=box)
    bs2.settings["static_builders"] = True
    bt2 = Backtest()
    bt2.run(bs2)
    assert bt2.stats["path"] == "l1-ipm" and bt2.stats["solved"] == len(rebdates)
    W = bt2.strategy.get_weights_df().to_numpy(dtype=float)
    xv = np.array(list(x0.values()))
    for i, (prob, sol) in enumerate(seen):
        assert sol.found and sol.extras.get("solver", "").startswith("device IPM")
        o = solve_qp(prob["P"], prob["q"], G=prob["G"], h=prob["h"], A=prob["A"], b=prob["b"],
                     lb=prob["lb"], ub=prob["ub"])
        assert abs(sol.obj - o.obj) <= 1e-6 * max(abs(o.obj), 1e-3), (sol.obj, o.obj)
        for w in (sol.x[:n], W[i]):
            assert np.abs(w).sum() <= 1.3 + 1e-7 and abs(w.sum() - 1) < 1e-8
            assert np.abs(w - xv).sum() <= 0.4 + 1e-7
        assert np.abs(W[i] - o.x[:n]).max() < 1e-6, (i, np.abs(W[i] - o.x[:n]).max())


@pytest.mark.gpu
def test_device_backtest_turnover_and_leverage_window_path():
    """n = 300 > window = 252: the per-asset-block IPM on the window form (coupling matrix
    from the weighted-SYRK kernel), mean-variance with shrinkage, long-short box, turnover
    budget + leverage, 12 daily dates in one batch; three dates against the oracle IPM on the
    reference's linearised problem built from the oracle's own covariance and mean."""
    import pandas as pd
    from oracle import ref_pipeline as rp
    from oracle.qp_ipm import solve_qp
    from porqua_amd.backtest import Backtest
    from porqua_amd.builders import OptimizationItemBuilder
    from porqua_amd.covariance import Covariance
    from porqua_amd.optimization import MeanVariance
    from porqua_amd.qp_problems import QuadraticProgram
    from porqua_amd.synthetic import factor_panel
    n, D, width = 300, 300, 252
    dates, R, yv, _ = factor_panel(D, n, seed=11)
    idx = pd.DatetimeIndex(dates)
    X = pd.DataFrame(R, index=idx, columns=[f"a{i}" for i in range(n)])
    y = pd.DataFrame({"bm": yv}, index=idx)
    rebdates = [str(d.date()) for d in idx[width + 5:width + 17]]
    w0 = np.random.default_rng(2).dirichlet(np.ones(n))
    x0 = dict(zip(X.columns, w0))

    def add_l1(bs, rebdate, **kw):
        bs.optimization.constraints.add_l1("turnover", rhs=0.5, x0=x0)
        bs.optimization.constraints.add_l1("leverage", rhs=1.2)

    opt = MeanVariance(covariance=Covariance(method="linear_shrinkage", lambda_covmat_regularization=0.1),
                       solver_name="mi355x", risk_aversion=1.0)
    bs = _service(opt, X, y, rebdates, extra=OptimizationItemBuilder(bibfn=add_l1), width=width,
                  box_kw={"box_type": "LongShort", "lower": -0.02, "upper": 0.05})
    bs.settings["static_builders"] = True
    bt = Backtest()
    bt.run(bs)
    assert bt.stats["path"] == "l1-ipm" and bt.stats["solved"] == len(rebdates)
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    for i in (0, 5, len(rebdates) - 1):
        e = X.index.get_loc(pd.Timestamp(rebdates[i]))
        Xw = R[e - width + 1:e + 1]
        S = rp.cov_pearson(Xw)
        S = S + 0.1 * np.mean(np.diag(S)) * np.eye(n)
        P, q = 2 * S, -rp.mean_geometric(Xw, None, None, None)
        qp = QuadraticProgram(P=P, q=q, A=np.ones((1, n)), b=np.ones(1), G=None, h=None,
                              lb=np.full(n, -0.02), ub=np.full(n, 0.05), params={"solver_name": "cvxopt"})
        qp.linearize_turnover_constraint(w0, 0.5)
        qp.linearize_leverage_constraint(N=n, leverage_budget=1.2)
        o = solve_qp(qp["P"], qp["q"], G=qp["G"], h=qp["h"], A=qp["A"], b=qp["b"], lb=qp["lb"], ub=qp["ub"])
        f = lambda x: 0.5 * x @ P @ x + q @ x                # noqa: E731
        # the linearised problem's optimal face is not a point (auxiliary variables), and the
        # oracle IPM's duality gap floors near 1e-7 relative there (its active-set refinement
        # does not apply): the device answer (feasible, checked below) may only be LOWER than
        # the oracle's by more than 1e-7, and sits within the north_star's 1e-6 bar either way
        fo, fw = f(o.x[:n]), f(W[i])
        assert fw - fo <= 1e-7 * max(abs(fo), 1e-6), (i, fw, fo)
        assert abs(fw - fo) <= 1e-6 * max(abs(fo), 1e-6), (i, fw, fo)
        assert np.abs(W[i] - o.x[:n]).max() < 1e-6, (i, np.abs(W[i] - o.x[:n]).max())
        assert np.abs(W[i]).sum() <= 1.2 + 1e-7 and np.abs(W[i] - w0).sum() <= 0.5 + 1e-7
        assert abs(W[i].sum() - 1) < 1e-8 and W[i].min() > -0.02 - 1e-8 and W[i].max() < 0.05 + 1e-8


@pytest.mark.gpu
def test_device_backtest_turnover_and_leverage_segment_split():
    """Turnover budget + leverage with a Pearson covariance (no ridge): the batched backtest
    takes the segment split on the ADMM engine (porqua_amd/l1seg.py; window path over
    [R, R, R], 3n = 300 > T + 3), 12 daily dates, long-short box, x0 with short positions;
    three dates against the oracle IPM on the reference's linearised problem
    (src/qp_problems.py:40-118).  n = 100 < T = 150: P = 2 Sigma is positive definite, so
    the optimum is unique and the weights are compared."""
    import pandas as pd
    from oracle import ref_pipeline as rp
    from oracle.qp_ipm import solve_qp
    from porqua_amd.backtest import Backtest
    from porqua_amd.builders import OptimizationItemBuilder
    from porqua_amd.optimization import MeanVariance
    from porqua_amd.qp_problems import QuadraticProgram
    from porqua_amd.synthetic import factor_panel
    n, D, width = 100, 180, 150
    dates, R, yv, _ = factor_panel(D, n, seed=13)
    idx = pd.DatetimeIndex(dates)
    X = pd.DataFrame(R, index=idx, columns=[f"a{i}" for i in range(n)])
    y = pd.DataFrame({"bm": yv}, index=idx)
    rebdates = [str(d.date()) for d in idx[width + 5:width + 17]]
    w0 = np.random.default_rng(4).dirichlet(np.ones(n)) * 1.3 - 0.3 / n
    x0 = dict(zip(X.columns, w0))

    def add_l1(bs, rebdate, **kw):
        bs.optimization.constraints.add_l1("turnover", rhs=0.5, x0=x0)
        bs.optimization.constraints.add_l1("leverage", rhs=1.25)

    opt = MeanVariance(solver_name="mi355x", risk_aversion=1.0)
    bs = _service(opt, X, y, rebdates, extra=OptimizationItemBuilder(bibfn=add_l1), width=width,
                  box_kw={"box_type": "LongShort", "lower": -0.04, "upper": 0.08})
    bs.settings["static_builders"] = True
    bs.settings["l1_segments"] = True
    bt = Backtest()
    bt.run(bs)
    assert bt.stats["path"] == "l1-segments" and bt.stats["solved"] == len(rebdates)
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    for i in (0, 6, len(rebdates) - 1):
        e = X.index.get_loc(pd.Timestamp(rebdates[i]))
        Xw = R[e - width + 1:e + 1]
        P, q = 2 * rp.cov_pearson(Xw), -rp.mean_geometric(Xw, None, None, None)
        qp = QuadraticProgram(P=P, q=q, A=np.ones((1, n)), b=np.ones(1), G=None, h=None,
                              lb=np.full(n, -0.04), ub=np.full(n, 0.08), params={"solver_name": "cvxopt"})
        qp.linearize_turnover_constraint(w0, 0.5)
        qp.linearize_leverage_constraint(N=n, leverage_budget=1.25)
        o = solve_qp(qp["P"], qp["q"], G=qp["G"], h=qp["h"], A=qp["A"], b=qp["b"], lb=qp["lb"], ub=qp["ub"])
        f = lambda x: 0.5 * x @ P @ x + q @ x                # noqa: E731
        fo, fw = f(o.x[:n]), f(W[i])
        assert abs(fw - fo) <= 1e-6 * max(abs(fo), 1e-6), (i, fw, fo)
        assert np.abs(W[i] - o.x[:n]).max() < 1e-5, (i, np.abs(W[i] - o.x[:n]).max())
        assert np.abs(W[i]).sum() <= 1.25 + 1e-7 and np.abs(W[i] - w0).sum() <= 0.5 + 1e-7
        assert abs(W[i].sum() - 1) < 1e-8 and W[i].min() > -0.04 - 1e-8 and W[i].max() < 0.08 + 1e-8
