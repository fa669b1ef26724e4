"""Host-side logic of the product package (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import ref_pipeline as rp
from porqua_amd import _lib, engine
from porqua_amd.backtest import shard_range
from porqua_amd.constraints import Constraints
from porqua_amd.synthetic import business_days, factor_panel
from tests.conftest import ROOT, load_golden


def test_window_rows_match_reference_semantics():
    g = load_golden("msci_panel")
    dates = g["dates"].astype("datetime64[D]")
    reb = dates[300::97]
    rows, tlen = engine.window_rows(dates, reb, 252)
    for b, d in enumerate(reb):
        assert np.array_equal(rows[b, :tlen[b]], rp.window_rows(dates, d, 252))
    # calendars with weekend rows: they are dropped, as src/builders.py:211 does
    cal = np.datetime64("2020-01-01") + np.arange(60)
    rows, tlen = engine.window_rows(cal, cal[[20, 59]], 10)
    for b, d in enumerate(cal[[20, 59]]):
        r = rp.window_rows(cal, d, 10)
        assert np.array_equal(rows[b, :tlen[b]], r) and len(r) < 10
    # a rebalance date before the data starts -> empty window
    rows, tlen = engine.window_rows(cal, [np.datetime64("2019-01-01")], 10)
    assert tlen[0] == 0


def test_slide_plan_groups_overlapping_windows():
    dates, _, _, _ = factor_panel(600, 3)
    # daily: every window is the previous one shifted by one row -> groups of 32
    rows, tlen = engine.window_rows(dates, dates[251:600], 252)
    gs, sh = engine.slide_plan(rows, tlen, group=32)
    assert list(gs[:3]) == [0, 32, 64] and gs[-1] == len(tlen)
    assert np.all(sh[gs[:-1]] <= 1) and np.all(np.delete(sh, gs[:-1]) == 1)
    # monthly stride 21 -> shift 21; beyond smax -> anchors only
    rows, tlen = engine.window_rows(dates, dates[251:600:21], 252)
    gs, sh = engine.slide_plan(rows, tlen)
    assert len(gs) == 2 and np.all(sh[1:] == 21)
    gs, sh = engine.slide_plan(rows, tlen, smax=20)
    assert len(gs) == len(tlen) + 1 and np.all(sh == 0)
    # every slid window really is its predecessor shifted by s rows
    cal = np.datetime64("2020-01-01") + np.arange(400)
    rows, tlen = engine.window_rows(cal, cal[100:160], 30)
    gs, sh = engine.slide_plan(rows, tlen)
    for d in np.flatnonzero(sh):
        T, s = tlen[d], sh[d]
        assert tlen[d - 1] == T and np.array_equal(rows[d, :T - s], rows[d - 1, s:T])
    # ragged (weekend-filtered) windows break groups
    assert len(gs) - 1 > 1 and sh[0] == 0


def test_business_days_and_panel_are_deterministic():
    d = business_days("2005-01-03", 10)
    assert ((d.astype(np.int64) + 3) % 7 < 5).all() and len(d) == 10
    a = factor_panel(50, 7)[1]
    b = factor_panel(50, 7)[1]
    assert np.array_equal(a, b)


def test_shard_range_covers_dates():
    for total in [1, 7, 4749, 10000]:
        for world in [1, 2, 3, 8]:
            parts = [shard_range(total, r, world) for r in range(world)]
            assert parts[0][0] == 0 and parts[-1][1] == total
            assert all(parts[i][1] == parts[i + 1][0] for i in range(world - 1))
            sizes = [e - s for s, e in parts]
            assert max(sizes) - min(sizes) <= 1


def test_qpbatch_layout_cpu():
    rng = np.random.default_rng(0)
    B, n = 3, 70
    P = rng.standard_normal((B, n, n))
    qb = engine.QPBatch.from_dense(P, rng.standard_normal((B, n)), A=np.ones((1, n)), b=np.ones(1),
                                   G=rng.random((2, n)), h=np.ones(2), lb=np.zeros(n), ub=np.ones(n),
                                   device=torch.device("cpu"))
    assert qb.ld == 128 and qb.mg == 3 and qb.shared
    assert np.array_equal(qb.P[:, :n, :n].numpy(), P) and float(qb.P[:, n:, :].abs().sum()) == 0
    assert qb.lg[0, 0] == qb.ug[0, 0] == 1.0 and np.isinf(qb.lg[0, 1].item()) and qb.ug[0, 2] == 1.0
    assert float(qb.lb[0, n:].abs().sum()) == 0 and float(qb.ub[0, n:].abs().sum()) == 0
    cs = qb.c_struct()
    assert cs.n == n and cs.ld == 128 and cs.Cg_stride == 0 and cs.P_stride == 128 * 128
    # per-problem constraints switch to strided storage
    qb2 = engine.QPBatch.from_dense(P, np.zeros((B, n)), A=np.ones((B, 1, n)), b=np.ones((B, 1)),
                                    device=torch.device("cpu"))
    assert not qb2.shared and qb2.c_struct().Cg_stride == qb2.Cg.stride(0)


def test_settings_from_params():
    s = engine.Settings.from_params({"eps_abs": 1e-7, "admm_max_iter": 50, "solver_name": "mi355x"})
    assert s.eps_abs == 1e-7 and s.max_iter == 50 and isinstance(s.max_iter, int)
    c = s.to_c()
    assert abs(c.eps_abs - 1e-7) < 1e-20 and c.max_iter == 50


def test_constraints_mirror_reference_shapes():
    """The reference's own known-answer test (test/tests_quadratic_program.py:28-58)."""
    g = load_golden("msci_panel")
    universe = pd.Index([str(c) for c in g["columns"]])
    c = Constraints(selection=universe)
    c.add_budget()
    c.add_box("LongOnly")
    rng = np.random.default_rng(1)
    c.add_linear(None, pd.Series(rng.random(universe.size), index=universe), "<=", 1)
    c.add_linear(None, pd.Series(rng.random(universe.size), index=universe), ">=", -1)
    c.add_linear(None, pd.Series(rng.random(universe.size), index=universe), "=", 0.5)
    sub = universe[: universe.size // 2]
    c.add_linear(pd.DataFrame(rng.random((3, sub.size)), columns=sub), None, pd.Series(np.repeat("=", 3)),
                 pd.Series(np.ones(3)), None)
    o = c.to_GhAb()
    assert o["G"].shape == (2, universe.size) and o["h"].shape == (2,)
    assert o["A"].shape == (5, universe.size) and o["b"].shape == (5,)
    o = c.to_GhAb(True)
    assert o["G"].shape == (2 + 2 * universe.size, universe.size) and o["h"].shape == (2 + 2 * universe.size,)


def test_constraints_values_match_reference_golden():
    g = load_golden("ghab")
    cols = [f"c{i}" for i in range(24)]
    u = pd.Index(cols)
    c = Constraints(selection=u)
    c.add_budget()
    c.add_box("LongOnly")
    c.add_linear(None, pd.Series(g["a1"], index=u), "<=", 1)
    c.add_linear(None, pd.Series(g["a2"], index=u), ">=", -1)
    c.add_linear(None, pd.Series(g["a3"], index=u), "=", 0.5)
    c.add_linear(pd.DataFrame(g["blk"], columns=u[:12]), None, pd.Series(np.repeat("=", 3)), pd.Series(np.ones(3)), None)
    for lbub, s in [(False, "0"), (True, "1")]:
        o = c.to_GhAb(lbub)
        for k in "GhAb":
            assert np.allclose(o[k], g[k + s])
    c2 = Constraints(selection=u)
    c2.add_budget()
    c2.add_box("LongShort")
    c2.add_linear(None, pd.Series(g["a3"], index=u), "=", 0.5)
    c2.add_linear(pd.DataFrame(g["blk"], columns=u[:12]), None, pd.Series(np.repeat("=", 3)), pd.Series(np.ones(3)), None)
    o = c2.to_GhAb(True)
    assert np.allclose(o["G"], g["G2"]) and np.allclose(o["h"], g["h2"])


def test_library_loads_and_exports_every_header_symbol():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "porqua_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(pq_\w+)\(", header, flags=re.M))
    assert declared and declared == set(_lib.exported_symbols())
    for name in declared:
        assert hasattr(lib, name)
    assert lib.pq_version() == 100
    # size query (host-only arithmetic, no GPU): dense and window layouts, bad arguments
    n, B, mg = 1000, 7, 1
    ld, mgp = 1024, 8
    dense = B * (8 * (ld * ld + (ld // 64) * 4096) + 16 * ld + 16 * (mgp + ld) + 8 + 12 + 64
                 + 8 * ((9 + mgp) * ld + 512))
    assert lib.pq_workspace_bytes(n, B, mg, 0, 0, 0) == dense
    win = lib.pq_workspace_bytes(n, B, mg, 1, 252, 256)
    assert win == dense - B * 8 * (ld * ld - 256 * 256 + (ld // 64 - 4) * 4096) + \
        B * (8 * (2 * 256 * 256 + 4 * 4096) + 12)
    assert lib.pq_workspace_bytes(0, B, mg, 0, 0, 0) == -1
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(rf"\bT {name}\b", nm), name


def test_ctypes_structs_match_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "porqua_hip.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pq_problem), sizeof(pq_state),'
                   ' sizeof(pq_settings), offsetof(pq_problem, lb), offsetof(pq_state, work),'
                   ' offsetof(pq_settings, refine_iters)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    exp = [ctypes.sizeof(_lib.PQProblem), ctypes.sizeof(_lib.PQState), ctypes.sizeof(_lib.PQSettings),
           _lib.PQProblem.lb.offset, _lib.PQState.work.offset, _lib.PQSettings.refine_iters.offset]
    assert got == exp


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.PorquaHipError):
        engine.default_device()
    from porqua_amd.qp_problems import QuadraticProgram
    n = 4
    qp = QuadraticProgram(P=np.eye(n), q=np.zeros(n), A=np.ones((1, n)), b=np.ones(1), lb=np.zeros(n),
                          ub=np.ones(n), params={"solver_name": "mi355x"})
    with pytest.raises(_lib.PorquaHipError):
        qp.solve()
    # more than 64 general rows (device IPM) and LAD (device LP IPM): no CPU fallback either
    big = QuadraticProgram(P=np.eye(n), q=np.zeros(n), G=np.ones((70, n)), h=np.ones(70),
                           params={"solver_name": "mi355x"})
    with pytest.raises(_lib.PorquaHipError):
        big.solve()
    import pandas as pd
    from porqua_amd.constraints import Constraints
    from porqua_amd.optimization import LAD
    from porqua_amd.optimization_data import OptimizationData
    idx = pd.bdate_range("2020-01-01", periods=30)
    X = pd.DataFrame(np.random.default_rng(0).normal(0, 0.01, (30, n)), index=idx, columns=list("abcd"))
    y = pd.DataFrame({"bm": X.mean(1)}, index=idx)
    cons = Constraints(selection=X.columns)
    cons.add_budget()
    lad = LAD(solver_name="mi355x", constraints=cons)
    lad.set_objective(OptimizationData(return_series=X, bm_series=y))
    with pytest.raises(_lib.PorquaHipError):
        lad.solve()


def test_lad_model_qpsolvers_matches_reference_lp():
    """LAD.model_qpsolvers (the non-engine route) builds the reference's LP
    (src/optimization.py:296-336) entry for entry: golden problems from tools/capture_lad.py."""
    import pandas as pd
    from porqua_amd.constraints import Constraints
    from porqua_amd.optimization import LAD
    from porqua_amd.optimization_data import OptimizationData
    from tests.conftest import load_golden
    p = load_golden("msci_panel")
    g = load_golden("msci_lad_ret")
    idx = pd.DatetimeIndex(p["dates"].astype("datetime64[D]"))
    cols = [str(c) for c in p["columns"]]
    X = pd.DataFrame(p["returns"], index=idx, columns=cols)
    y = pd.DataFrame({"bm": p["bm"]}, index=idx)
    for i in (0, 11):
        e = idx.searchsorted(pd.Timestamp(str(g["rebdates"][i])), side="right")
        cons = Constraints(selection=cols)
        cons.add_budget()
        cons.add_box("LongOnly", upper=0.3)
        lad = LAD(solver_name="cvxopt", use_level=False, constraints=cons)
        lad.set_objective(OptimizationData(return_series=X.iloc[e - 252:e], bm_series=y.iloc[e - 252:e]))
        lad.model_qpsolvers()
        m = lad.model
        assert np.array_equal(m["q"], g["q"][i]) and np.allclose(m["A"], g["A"][i], rtol=1e-13, atol=0)
        assert np.allclose(m["b"], g["b"][i], rtol=1e-13, atol=0)
        assert np.array_equal(m["lb"], g["lb"][i]) and np.array_equal(m["ub"], g["ub"][i])
        assert not np.any(m["P"]) and m["G"] is None


def test_api_objects_construct_without_gpu():
    from porqua_amd.backtest import Backtest, BacktestService
    from porqua_amd.builders import OptimizationItemBuilder, SelectionItemBuilder, bibfn_selection_data
    from porqua_amd.covariance import Covariance
    from porqua_amd.optimization import (EmptyOptimization, LeastSquares, MeanVariance, QEQW,
                                         WeightedLeastSquares)
    for cls in (LeastSquares, MeanVariance, QEQW, WeightedLeastSquares, EmptyOptimization):
        o = cls(solver_name="mi355x")
        assert o.params["solver_name"] == "mi355x"
    assert LeastSquares().params["solver_name"] == "mi355x" and LeastSquares(verbose=False).params["verbose"] is False
    mv = MeanVariance(covariance=Covariance(method="linear_shrinkage", lambda_covmat_regularization=0.1))
    assert mv.params["risk_aversion"] == 1 and mv.covariance.spec["method"] == "linear_shrinkage"
    bs = BacktestService(data={}, selection_item_builders={"d": SelectionItemBuilder(bibfn=bibfn_selection_data)},
                         optimization_item_builders={}, optimization=mv, rebdates=[])
    Backtest().run(bs)


def test_group_plan_joins_identical_windows_of_a_sweep():
    """A risk-aversion sweep repeats every date's window; the grouped-ADMM plan joins the
    repeats (shift 0, same union), the sliding-K1 plan does not."""
    dates, _, _, _ = factor_panel(400, 3)
    rows, tlen = engine.window_rows(dates, dates[[300, 390]], 120)   # 90-row gap: no slide
    rep_rows, rep_tlen = np.repeat(rows, 6, axis=0), np.repeat(tlen, 6)
    gs, sh = engine.slide_plan(rep_rows, rep_tlen, group=16, smin=0)
    assert list(gs) == [0, 6, 12] and np.all(sh == 0)
    gs1, _ = engine.slide_plan(rep_rows, rep_tlen, group=16)
    assert len(gs1) - 1 == 12
    gp = engine.GroupPlan(rep_rows, rep_tlen, torch.device("cpu"))   # 12 problems: groups of <= 4
    assert gp.ok and list(gp.gdates.numpy()) == [0, 4, 6, 10, 12]
    assert np.all(gp.ucnt.numpy() == 120) and np.all(gp.uoff.numpy() == 0)


def test_kkt_certificate_accepts_oracle_and_rejects_perturbed():
    from oracle.qp_ipm import solve_qp
    from tests.kkt import kkt_residuals
    rng = np.random.default_rng(3)
    n = 40
    X = rng.normal(0, 0.02, (30, n))
    P = 2 * X.T @ X + 1e-4 * np.eye(n)
    q = -rng.normal(0, 0.01, n)
    G = (rng.random((3, n)) < 0.4).astype(float)
    h = np.full(3, 0.3)
    o = solve_qp(P, q, G=G, h=h, A=np.ones((1, n)), b=np.ones(1), lb=np.zeros(n), ub=np.full(n, 0.2))
    y = np.concatenate([np.atleast_1d(o.y), np.atleast_1d(o.z)])
    k = kkt_residuals(P, q, o.x, A=np.ones((1, n)), b=np.ones(1), G=G, h=h, lb=np.zeros(n),
                      ub=np.full(n, 0.2), y=y, z_box=o.z_box)
    assert max(k.values()) < 1e-9, k
    xp = o.x.copy()
    xp[:2] += np.array([1e-4, -1e-4])
    k2 = kkt_residuals(P, q, xp, A=np.ones((1, n)), b=np.ones(1), G=G, h=h, lb=np.zeros(n),
                       ub=np.full(n, 0.2), y=y, z_box=o.z_box)
    assert max(k2.values()) > 1e-7


def _loop_slide_plan(rows, tlen, group, smax, smin):
    """Direct restatement of engine.slide_plan's contract: d joins d-1 when its window is
    that window shifted by smin <= s <= smax rows (same length), groups of <= ``group``."""
    B = len(tlen)
    shift = np.zeros(B, dtype=np.int32)
    gs = [0] if B else []
    cnt = 1
    for d in range(1, B):
        tp, tc = int(tlen[d - 1]), int(tlen[d])
        prev, cur = rows[d - 1, :tp], rows[d, :tc]
        s = int((prev < cur[0]).sum()) if tc else 0
        ok = tp == tc and tc > 1 and smin <= s <= smax and np.array_equal(prev[s:], cur[:tc - s])
        if ok:
            shift[d] = s
        if not ok or cnt == group:
            gs.append(d)
            cnt = 0
        cnt += 1
    gs.append(B)
    return np.asarray(gs, dtype=np.int32), shift


def test_planners_match_their_contracts_on_random_calendars():
    """window_rows (vs the oracle's per-date restatement of src/builders.py:208-211),
    slide_plan (vs a per-date loop) and GroupPlan (every date's window is its union slice
    [uoff, uoff + T), unions within umax) on calendars with weekends, gaps, repeated
    rebalance dates, descending or shuffled rebalance dates and short histories."""
    import torch
    rng = np.random.default_rng(11)
    for trial in range(30):
        n = int(rng.integers(30, 1500))
        cal = np.arange(np.datetime64("2003-01-01"), np.datetime64("2003-01-01") + n)
        if trial % 3:
            cal = cal[((cal.astype("int64") + 3) % 7) < 5]
        if trial % 2:
            cal = cal[rng.random(len(cal)) < 0.93]
        if len(cal) < 3:
            continue
        T = int(rng.integers(2, 120))
        reb = cal[int(rng.integers(0, min(len(cal) - 1, T + 3))):][::int(rng.choice([1, 1, 3, 21]))]
        if trial % 4 == 0:
            reb = np.repeat(reb, int(rng.integers(1, 4)))
        if trial % 5 == 1:     # descending rebalance dates: a later window starts earlier
            reb = reb[::-1].copy()
        elif trial % 5 == 3:   # shuffled (the slide plan must not take them as identical)
            reb = reb[rng.permutation(len(reb))]
        rows, tlen = engine.window_rows(cal, reb, T)
        for b in range(0, len(reb), max(1, len(reb) // 17)):
            assert np.array_equal(rows[b, :tlen[b]], rp.window_rows(cal, reb[b], T))
        for group, smax, smin in ((32, 64, 1), (16, 64, 0), (3, 5, 0)):
            gs, sh = engine.slide_plan(rows, tlen, group, smax, smin)
            gs2, sh2 = _loop_slide_plan(rows, tlen, group, smax, smin)
            assert np.array_equal(gs, gs2) and np.array_equal(sh, sh2)
        gp = engine.GroupPlan(rows, tlen, torch.device("cpu"), gmax=16, gmin=16)
        if not gp.ok:
            continue
        gd, ur, uc, uo = (gp.gdates.numpy(), gp.urows.numpy(), gp.ucnt.numpy(), gp.uoff.numpy())
        assert gd[0] == 0 and gd[-1] == len(tlen) and (np.diff(gd) >= 1).all() and (uc <= gp.umax).all()
        for g in range(gp.ngroups):
            for d in range(gd[g], gd[g + 1]):
                t = int(tlen[d])
                assert np.array_equal(ur[g, uo[d]:uo[d] + t], rows[d, :t])


def test_sparse_columns_of_group_rows():
    """engine._sparse_columns: budget + 0/1 sector rows -> per-column (row, value) lists with
    -1 padding; dense or few rows -> none (the grouped ADMM then reads Cg densely)."""
    import torch
    n = 10
    sec = np.array([0, 1, 2, 0, 1, 2, 3, 3, 0, 1])
    G = np.stack([(sec == g).astype(float) for g in range(4)])
    qb = engine.QPBatch.from_dense(None, None, n=n, A=np.ones((1, n)), b=np.ones(1), G=G, h=np.full(4, 0.5),
                                   lb=np.zeros(n), ub=np.ones(n), device=torch.device("cpu"))
    rows, vals, nzmax = engine._sparse_columns(qb)
    assert nzmax == 2 and rows.shape == (qb.ld, 2)
    C = qb.Cg[0, :qb.mg, :n].numpy()
    for i in range(n):
        dense = np.zeros(qb.mg)
        for r, v in zip(rows[i].tolist(), vals[i].tolist()):
            if r >= 0:
                dense[r] = v
        assert np.array_equal(dense, C[:, i])
    assert (rows[n:] == -1).all()
    qb2 = engine.QPBatch.from_dense(None, None, n=n, A=np.ones((1, n)), b=np.ones(1), G=np.ones((4, n)),
                                    h=np.full(4, 0.5), lb=np.zeros(n), ub=np.ones(n), device=torch.device("cpu"))
    assert engine._sparse_columns(qb2)[2] == 0     # 5 nonzeros per column: dense reads


def test_trailing_window_slice_matches_the_boolean_mask():
    """builders._upto (one positional slice on a sorted DatetimeIndex) returns exactly
    data[data.index <= rebdate].tail(width) (src/builders.py:188-251), for dates inside,
    before and after the panel, dates between rows, any width, and an unsorted index."""
    import pandas as pd
    from porqua_amd import builders
    idx = pd.bdate_range("2020-01-01", periods=300)
    df = pd.DataFrame(np.arange(600.0).reshape(300, 2), index=idx, columns=["a", "b"])
    for data in (df, df.iloc[::-1], df["a"]):
        for date in ("2019-06-01", "2020-01-01", "2020-03-07", str(idx[150].date()), str(idx[-1].date()),
                     "2030-01-01"):
            for width in (1, 21, 252, 1000, None):
                ref = data[data.index <= date]
                ref = ref.tail(width) if width is not None else ref
                assert builders._upto(data, date, width).equals(ref), (date, width)


def test_single_binary_filter_selection():
    import pandas as pd
    from porqua_amd.selection import Selection
    s = Selection()
    s.add_filtered("data", pd.Series([1, 0, 1, 1], index=list("abcd"), name="binary"))
    assert list(s.selected) == ["a", "c", "d"] and isinstance(s.selected, pd.Index)
    s.add_filtered("more", pd.Series([1, 1, 0, 1], index=list("abcd"), name="binary"))
    assert list(s.selected) == ["a", "d"]


def test_panel_upload_resolves_the_device_on_the_calling_thread(monkeypatch):
    """_PanelUpload asks for the device on the caller's thread (torch's current device is
    per host thread: a worker would see device 0, not the rank's set_device choice) and copies
    to that device on the worker."""
    import threading
    from porqua_amd import backtest as bt
    seen = []

    def fake_device():
        seen.append(threading.current_thread())
        return torch.device("cpu")

    monkeypatch.setattr(engine, "default_device", fake_device)
    frame = pd.DataFrame(np.arange(12.0).reshape(4, 3))
    up = bt._PanelUpload(frame)
    out = up.result()
    assert seen == [threading.current_thread()]
    assert out.device.type == "cpu" and np.array_equal(out.numpy(), frame.to_numpy())


def test_loose_stop_eps_rule():
    """engine.loose_stop_eps: centred windows take eps_grouped; tracking windows take
    eps_grouped_tracking, or eps_grouped_tracking_small (off by default) for batches of at
    most small_batch dates (the notebook's monthly run), or eps_grouped_tracking_wide with more
    than 4 general rows (config 4's sector caps); eps_grouped = 0 turns every loose stop off."""
    from porqua_amd import engine
    s = engine.Settings()
    assert engine.loose_stop_eps(s, True, 4749) == s.eps_grouped
    assert engine.loose_stop_eps(s, False, 4544) == 0.0
    assert s.eps_grouped_tracking_small == 0.0 and engine.loose_stop_eps(s, False, 13) == 0.0
    assert engine.loose_stop_eps(s, False, 13, mg=21) == s.eps_grouped_tracking_wide   # small wide batch
    sm = engine.Settings(eps_grouped_tracking_small=1e-2)
    assert engine.loose_stop_eps(sm, False, 13) == 1e-2
    assert engine.loose_stop_eps(sm, False, sm.small_batch) == 1e-2
    assert engine.loose_stop_eps(sm, False, sm.small_batch + 1) == 0.0
    off = engine.Settings(eps_grouped=0.0)
    assert engine.loose_stop_eps(off, False, 13) == 0.0 and engine.loose_stop_eps(off, True, 13) == 0.0
    assert engine.loose_stop_eps(s, False, 9749, mg=21) == s.eps_grouped_tracking_wide > 0.0
    assert engine.loose_stop_eps(s, False, 9749, mg=4) == 0.0
    assert engine.loose_stop_eps(off, False, 9749, mg=21) == 0.0
    own = engine.Settings(eps_grouped_tracking=3e-2)
    assert engine.loose_stop_eps(own, False, 13) == 3e-2 and engine.loose_stop_eps(own, False, 4544) == 3e-2


def test_sweep_plan_groups_and_applicability():
    """engine.SweepPlan (the risk-aversion groups of pq_admm_lr_sweep): rows of up to 64
    problems, a longer row split, and the kernel's shape conditions."""
    sp = engine.SweepPlan([40, 70, 64], "cpu")
    assert sp.gdates.tolist() == [0, 40, 104, 110, 174] and sp.ngroups == 4
    assert engine.SweepPlan([], "cpu").ngroups == 0
    n = 300
    qb = engine.QPBatch(n, 174, 1, device="cpu", P=torch.empty(0, dtype=torch.float64))

    class LR:
        tmax = 252
    assert sp.applicable(qb, LR(), 256)
    LR.tmax = 300                       # window beyond the kernel's 256 rows
    assert not sp.applicable(qb, LR(), 256)
    LR.tmax = 252
    assert not sp.applicable(qb, LR(), 320)   # capacitance beyond k_ld 256
    q5 = engine.QPBatch(n, 174, 5, device="cpu", P=torch.empty(0, dtype=torch.float64))
    assert not sp.applicable(q5, LR(), 256)   # more than 4 general rows
    qs = engine.QPBatch(n, 174, 1, device="cpu", shared_constraints=False, P=torch.empty(0, dtype=torch.float64))
    assert not sp.applicable(qs, LR(), 256)   # per-problem rows / boxes
    need = _lib.load().pq_sweep_scratch_doubles(5000, 4096, 64)
    assert need == 4096 * 80 + 64 * 20 * 64 * (256 + 16) + 64 * 256 * 64 + 64


@pytest.mark.parametrize("counts", [[1], [64], [65], [128], [129], [70, 3, 64]])
def test_sweep_plan_never_emits_a_group_beyond_64(counts):
    """pq_admm_lr_sweep's unchecked precondition gdates[g + 1] - gdates[g] <= 64 (a group's
    problems are the 64 MFMA columns of one workgroup): the plan cuts longer rows, covers
    every problem once, in order, and never joins two rows."""
    sp = engine.SweepPlan(counts, "cpu")
    gd = np.asarray(sp.gdates.tolist())
    sizes = np.diff(gd)
    assert gd[0] == 0 and gd[-1] == sum(counts) and sp.ngroups == len(sizes)
    assert sizes.min() >= 1 and sizes.max() <= engine.SweepPlan.GMAX == 64
    assert sp.ngroups == sum(-(-c // 64) for c in counts)
    assert set(np.cumsum(counts).tolist()) <= set(gd.tolist())   # no group straddles two rows


def test_window_rows_without_rebalance_dates():
    """No rebalance dates on a non-empty calendar: empty plans (the full-window fast path
    once took the minimum of an empty tlen)."""
    dates, _, _, _ = factor_panel(40, 4)
    for reb in ([], np.array([], dtype="datetime64[D]")):
        rows, tlen = engine.window_rows(dates, reb, 10)
        assert rows.shape == (0, 1) and rows.dtype == np.int32
        assert tlen.shape == (0,) and tlen.dtype == np.int32
    rows, tlen = engine.window_rows(dates, dates[[9, 20]], 10)   # (the fast path itself still runs)
    assert tlen.tolist() == [10, 10] and np.array_equal(rows[1], np.arange(11, 21))


# ---- engine.lowrank_route: which kernels solve_lowrank runs, on CPU tensors ------------------

def _route_problem(mg=1, shared=True, rows_kind="sparse", uniform=True, centred=True, cus=256):
    """tests/test_gcap_gpu.py::_problem at n = 300, T = 60, D = 40, stride 1, on the CPU: the
    batch, a stub of the window (what the route reads of it), the GroupPlan and a Workspace."""
    from types import SimpleNamespace
    n, T, D, cpu = 300, 60, 40, torch.device("cpu")
    ends = list(range(T + 5, T + 5 + D))
    dates, R, _, sec = factor_panel(max(ends) + 1, n)
    rows, tlen = engine.window_rows(dates, dates[ends], T)
    qb = engine.QPBatch(n, D, mg, device=cpu, shared_constraints=shared, P=torch.empty(0, dtype=torch.float64))
    qb.P = None
    qb.lb[:, :n], qb.ub[:, :n] = 0.0, 0.2
    qb.lb[:, n:] = qb.ub[:, n:] = 0.0
    if mg:
        qb.Cg[:, 0, :n] = 1.0                       # the budget
        qb.lg[:, 0] = qb.ug[:, 0] = 1.0
    for r in range(1, mg):                          # 0/1 sector rows (disjoint) or dense rows
        qb.Cg[:, r, :n] = torch.from_numpy((sec == r - 1).astype(float)) if rows_kind == "sparse" else 1.0 + r
        qb.ug[:, r] = 0.3
    qb.p_scale = torch.full((D,), 2.0, dtype=torch.float64)
    if not uniform:
        qb.p_scale[1::2] = 4.0
    mu = torch.zeros((D, qb.ld), dtype=torch.float64) if centred else None
    lr = SimpleNamespace(tmax=T, panel=SimpleNamespace(R=torch.from_numpy(R)), mu=mu, w_scale=None)
    gp = engine.GroupPlan(rows, tlen, cpu, cus=cus)
    ws = engine.Workspace(qb, dense=False)
    assert gp.ok and engine.lowrank_applicable(qb, lr) and engine.grouped_applicable(qb, lr, gp, ws)
    return qb, lr, gp, ws


def _route(qb, lr, gp, ws, settings=None, **kw):
    return engine.lowrank_route(qb, lr, ws, gp, settings or engine.Settings(), **kw)


def _route_fields(r):
    return (r.capacitance, r.admm, r.polish, r.band, r.loose_eps, r.loose_min_iter, r.sync_free)


def test_lowrank_route_table():
    """The whole route of solve_lowrank for each combination of caller flags and problem facts
    the host code distinguishes (expected values: the conditions of the code before the route
    was made explicit, the same the "which kernel ran" assertions of tests/test_gcap_gpu.py,
    tests/test_admm_iterates_gpu.py and tests/test_sweep_admm_gpu.py pin on the device)."""
    d = engine.Settings()
    assert (d.eps_grouped, d.min_iter_grouped) == (0.5, 7)
    # 1. defaults: the group capacitance on its own plan (20-date groups), grouped polish, the loose stop
    #    for centred windows, sync_free honoured
    qb, lr, gp, ws = _route_problem(cus=1)
    assert (gp.ngroups, gp.ucnt_max, gp.corr_max) == (3, 73, 14) and gp.sizes.tolist() == [14, 14, 12]
    g32 = gp.gcap_plan()
    assert g32 is not gp and g32.sizes.tolist() == [20, 20]
    r = _route(qb, lr, gp, ws)
    assert r.grouped and r.plan is g32 and r.band_wmin == max(g32.span_max, gp.span_max) == 60 + 19
    assert _route_fields(r) == ("group", "gcap", "grouped", True, 0.5, 7, False)
    assert _route(qb, lr, gp, ws, sync_free=True).sync_free
    #    uncentred (tracking) windows keep eps_abs / eps_rel
    qb_u, lr_u, gp_u, ws_u = _route_problem(centred=False)
    assert (gp_u.ngroups, gp_u.ucnt_max, gp_u.corr_max) == (10, 63, 4) and gp_u.gcap_plan() is gp_u
    assert _route_fields(_route(qb_u, lr_u, gp_u, ws_u)) == ("group", "gcap", "grouped", True, 0.0, 0, False)
    # 2. gcap=False: the grouped kernel's fused form on the band capacitance; no loose stop
    #    (eps_grouped_percap is off), a sync_free request is refused
    r = _route(qb, lr, gp, ws, gcap=False, sync_free=True)
    assert r.plan is gp and r.band_wmin == gp.span_max   # (wide_polish: the polish plan's unions)
    assert _route_fields(r) == ("band", "grouped-fused", "grouped", True, 0.0, 0, False)
    r = _route(qb, lr, gp, ws, engine.Settings(eps_grouped_percap=True), gcap=False)
    assert (r.admm, r.loose_eps, r.loose_min_iter) == ("grouped-fused", 0.5, 7)
    assert _route(qb, lr, gp, ws, gcap=False, wide_polish=False).band_wmin == 0
    # 3. fuse=False: the unfused grouped kernel, no group capacitance
    r = _route(qb, lr, gp, ws, fuse=False, sync_free=True)
    assert r.plan is gp and _route_fields(r) == ("band", "grouped-unfused", "grouped", True, 0.0, 0, False)
    # 4. groups=None: the per-problem ADMM and the per-date polish
    r = _route(qb, lr, None, ws, sync_free=True)
    assert not r.grouped and r.plan is None and r.band_wmin == 0
    assert _route_fields(r) == ("band", "per-problem", "per-date", True, 0.0, 0, False)
    #    ... the per-date polish also without the grouped polish, on the group capacitance
    assert _route_fields(_route(qb, lr, gp, ws, grouped_polish=False, sync_free=True)) == \
        ("group", "gcap", "per-date", True, 0.0, 0, False)
    # 5. per-problem constraints: the direct capacitance, no band, no gcap, no fused form
    qb5, lr5, gp5, ws5 = _route_problem(shared=False)
    r = _route(qb5, lr5, gp5, ws5, sync_free=True)
    assert r.plan is gp5 and _route_fields(r) == ("direct", "grouped-unfused", "grouped", False, 0.0, 0, False)
    assert _route_fields(_route(qb, lr, gp, ws, band=False)) == ("direct", "grouped-unfused", "grouped", False, 0.0, 0,
                                                                  False)
    # 6. the dates of a group differ in c = p_scale w_scale (a risk-aversion sweep) and a
    #    SweepPlan is given: the sweep kernel on the band capacitance, no group capacitance
    qb6, lr6, gp6, ws6 = _route_problem(uniform=False)
    sp = engine.SweepPlan([4] * 10, qb6.device, q_shared=True)
    r = _route(qb6, lr6, gp6, ws6, sweep=sp, sync_free=True)
    assert r.plan is gp6 and _route_fields(r) == ("band", "sweep", "grouped", True, 0.0, 0, False)
    assert _route(qb6, lr6, gp6, ws6).admm == "grouped-fused"            # (no SweepPlan)
    assert _route(qb, lr, gp, ws, sweep=sp).admm == "gcap"               # (uniform groups: gcap wins)
    assert _route(qb6, lr6, gp6, ws6, sweep=sp, fuse=False).admm == "grouped-unfused"
    old = engine.SWEEP_ADMM
    try:
        engine.SWEEP_ADMM = False
        assert _route(qb6, lr6, gp6, ws6, sweep=sp).admm == "grouped-fused"
    finally:
        engine.SWEEP_ADMM = old
    # 7. as 6 with the per-date eigendecompositions: "eig", the sweep kernel still chosen
    r = _route(qb6, lr6, gp6, ws6, sweep=sp, eig=object())
    assert _route_fields(r) == ("eig", "sweep", "grouped", True, 0.0, 0, False)
    assert _route(qb, lr, gp, ws, eig=object()).admm == "grouped-fused"  # (eig: never the group capacitance)
    # 8. more than 4 general rows: gcap only in the column-sparse form (budget + 8 disjoint 0/1 rows)
    qb8, lr8, gp8, ws8 = _route_problem(mg=9)
    r = _route(qb8, lr8, gp8, ws8)
    assert r.sparse_cols[2] == 2 and _route_fields(r) == ("group", "gcap", "grouped", True, 0.5, 7, False)
    qb8u, lr8u, gp8u, ws8u = _route_problem(mg=9, centred=False)       # tracking, wide form: its own loose stop
    assert d.eps_grouped_tracking_wide == 1e-2
    assert _route_fields(_route(qb8u, lr8u, gp8u, ws8u)) == ("group", "gcap", "grouped", True, 1e-2, 7, False)
    qb8d, lr8d, gp8d, ws8d = _route_problem(mg=5, rows_kind="dense")
    r = _route(qb8d, lr8d, gp8d, ws8d)
    assert r.sparse_cols[2] == 0 and _route_fields(r) == ("band", "grouped-fused", "grouped", True, 0.0, 0, False)
    # 9. polish=False (or settings.polish = 0): no polish, no loose stop, sync_free refused
    for kw in (dict(polish=False), dict(settings=engine.Settings(polish=0))):
        r = _route(qb, lr, gp, ws, sync_free=True, **kw)
        assert r.plan is g32 and _route_fields(r) == ("group", "gcap", "none", True, 0.0, 0, False)
    # 10. engine.GCAP_MAX_DATES = 16 (read when the plan is first asked for): the plan is groups itself
    qb10, lr10, gp10, ws10 = _route_problem(cus=1)
    old = engine.GCAP_MAX_DATES
    try:
        engine.GCAP_MAX_DATES = 16
        r = _route(qb10, lr10, gp10, ws10)
    finally:
        engine.GCAP_MAX_DATES = old
    assert r.plan is gp10 and _route_fields(r) == ("group", "gcap", "grouped", True, 0.5, 7, False)
    #     ... and engine.GCAP32_WIDE = False keeps the 16-date groups for the column-sparse form only
    qbw, lrw, gpw, wsw = _route_problem(mg=9, cus=1)
    old = engine.GCAP32_WIDE
    try:
        engine.GCAP32_WIDE = False
        assert _route(qbw, lrw, gpw, wsw).plan is gpw and _route(qb, lr, gp, ws).plan is g32
    finally:
        engine.GCAP32_WIDE = old
    assert _route(qbw, lrw, gpw, wsw).plan is gpw.gcap_plan() is not gpw
    # 11. shared rows, but box rows that do not share one rho -- the split box of a turnover term around a
    #     previous portfolio at its bounds (fixed [0, 0] variables next to ordinary ones), a one-sided row, or a
    #     free row among ordinary ones: the route of 5 (tests/test_window_mixed_gpu.py pins it on the device)
    n11 = qb.n
    for lo, up, uniform in ((0.0, 0.0, False), (-np.inf, np.inf, False), (0.0, np.inf, True)):
        qb11, lr11, gp11, ws11 = _route_problem()
        qb11.lb[0, 3:n11:5], qb11.ub[0, 3:n11:5] = lo, up
        assert engine._uniform_box(qb11) == uniform
        r = _route(qb11, lr11, gp11, ws11, sync_free=True)
        if uniform:   # (a one-sided row still takes rho: the band form stays)
            assert r.capacitance == "group"
            continue
        assert r.plan is gp11 and _route_fields(r) == ("direct", "grouped-unfused", "grouped", False, 0.0, 0, False)
        assert _route_fields(_route(qb11, lr11, None, ws11)) == ("direct", "per-problem", "per-date", False, 0.0, 0, False)
    # 12. no box at all: one D for every asset, so the band and the group capacitance stay (the window form
    #     remains applicable: test_free_rows_and_boxless_batches_are_certified holds it to its certificate)
    qb12, lr12, gp12, ws12 = _route_problem()
    qb12.lb = qb12.ub = None
    qb12.has_box = False
    assert engine.lowrank_applicable(qb12, lr12) and engine._uniform_box(qb12)
    assert _route_fields(_route(qb12, lr12, gp12, ws12)) == ("group", "gcap", "grouped", True, 0.5, 7, False)


def test_workspace_declares_what_the_engine_sets():
    """Every attribute solve_lowrank later sets exists (None) on a new Workspace."""
    qb, _, _, ws = _route_problem()
    for name in ("sweep_admm", "band_shape", "gcap_groups", "pg_fallback", "_pg_pass", "_sf_flag", "_pg_rec",
                 "_gcap", "_pgw"):
        assert name in vars(ws) and getattr(ws, name) is None, name
