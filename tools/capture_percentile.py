#!/usr/bin/env python3
"""Capture golden vectors for the quantile portfolios (PercentilePortfolios,
``src/optimization.py:356-417``) from the PorQua reference (run in the build container only).

Imports the reference's ``optimization.py`` / ``mean_estimation.py`` / ``backtest.py``
read-only through ``capture_golden``'s stub set-up and records, on the msci panel
(``tests/golden/msci_panel.npz``), into ``tests/golden/msci_percentile.npz``:

(a) for a handful of windows: the estimator's scores (``MeanEstimator(method='geometric',
    n_mom=252, n_rev=21)``) and the reference ``solve()`` thresholds, long-short weights and
    per-bucket member masks for N in {1, 3, 5};
(b) the reference walkthrough's own backtest (``src/_quick_and_dirty_interactive_testing.py``,
    last section): rebalance dates every 63 rows after 2010-01-01, ``width=365*3`` with the
    weekend filter, quintiles, run through the reference's serial ``Backtest.run`` with
    ``append_custom(['w_dict'])``; per date the scores, the long-short weights and the bucket
    masks read back from ``Backtest.output``.

Two things are asserted and recorded.  No score is exactly zero, so the reference's unseeded
``np.random.normal`` step (``src/optimization.py:393``) never fires and the fixture is
reproducible.  And the smallest relative gap between any threshold with gamma != 0 (a
threshold strictly between two scores) and any score of its date: bucket membership computed
from scores that differ from pandas' in the last bits is the reference's only while that gap
is far above FP64 rounding.  Dates of (b) with a gap below 1e-9 are dropped (at most 5 %).

Usage:  python tools/capture_percentile.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import capture_golden as cg  # noqa: E402  (stubs qpsolvers, puts the reference on sys.path)

from backtest import Backtest, BacktestService, append_custom  # noqa: E402  (reference)
from builders import (  # noqa: E402
    OptimizationItemBuilder, SelectionItemBuilder, bibfn_box_constraints, bibfn_bm_series,
    bibfn_budget_constraint, bibfn_return_series, bibfn_selection_data)
from mean_estimation import MeanEstimator  # noqa: E402
from optimization import PercentilePortfolios  # noqa: E402

WIDTH = 365 * 3
N_MOM, N_REV = 252, 21
STRIDE = 63
MIN_GAP = 1e-9
MAX_DROP = 0.05


def estimator():
    return MeanEstimator(method="geometric", scalefactor=1, n_mom=N_MOM, n_rev=N_REV)


def score_gap(x: np.ndarray, N: int) -> float:
    """Smallest relative distance between a threshold with gamma != 0 and a score of x."""
    n = len(x)
    v = (n - 1) * (np.linspace(0, 100, N + 1) / 100)
    th = np.percentile(x, np.linspace(0, 100, N + 1))
    gap = np.inf
    for t in np.flatnonzero(v != np.floor(v)):
        gap = min(gap, float(np.min(np.abs(th[t] - x) / np.maximum(np.abs(th[t]), np.abs(x)))))
    return gap


def solve_reference(scores: pd.Series, N: int):
    """The reference solve() of one raw score vector: (th, weights, masks [N, n])."""
    opt = PercentilePortfolios(estimator=None, n_percentiles=N)
    opt.objective = {"scores": -scores}
    assert opt.solve() is True
    names = list(scores.index)
    w = np.array([opt.results["weights"][k] for k in names], dtype=np.float64)
    masks = np.array([[k in opt.results["w_dict"][i].index for k in names] for i in range(1, N + 1)])
    for i in range(1, N + 1):
        assert np.all(opt.results["w_dict"][i].values == 1 / masks[i - 1].sum())
    th = np.percentile((-scores).to_numpy(), np.linspace(0, 100, N + 1))
    return th, w, masks


def main():
    p = np.load(os.path.join(cg.OUT, "msci_panel.npz"))
    dates = pd.DatetimeIndex(p["dates"].astype("datetime64[D]"))
    names = [str(c) for c in p["columns"]]
    X = pd.DataFrame(p["returns"], index=dates, columns=names)
    y = pd.DataFrame({"bm": p["bm"]}, index=dates)
    out = {"width": np.int64(WIDTH), "n_mom": np.int64(N_MOM), "n_rev": np.int64(N_REV)}

    # ---- (a) single windows ------------------------------------------------------------
    a_dates = [str(d.date()) for d in dates[dates > "2003-01-01"][::701]][:8]
    a_scores, a_gap = [], []
    a_out = {N: ([], [], []) for N in (1, 3, 5)}
    for d in a_dates:
        win = X[X.index <= d].tail(WIDTH)
        win = win[win.index.dayofweek < 5]
        s = estimator().estimate(X=win)
        assert not (s == 0).any(), "a zero score: the reference's RNG step would fire"
        a_scores.append(s.to_numpy(dtype=np.float64))
        a_gap.append(min(score_gap(-s.to_numpy(), N) for N in (3, 5)))
        for N, (ths, ws, ms) in a_out.items():
            th, w, masks = solve_reference(s, N)
            ths.append(th), ws.append(w), ms.append(masks)
    assert min(a_gap) >= MIN_GAP, a_gap
    out.update(a_dates=np.array(a_dates), a_scores=np.array(a_scores), a_gap=np.array(a_gap))
    for N, (ths, ws, ms) in a_out.items():
        out[f"a_th_{N}"], out[f"a_w_{N}"], out[f"a_masks_{N}"] = np.array(ths), np.array(ws), np.array(ms)

    # ---- (b) the walkthrough's backtest --------------------------------------------------
    rebdates = dates[dates > "2010-01-01"][::STRIDE].strftime("%Y-%m-%d").tolist()
    seen = {}

    def append_fun(backtest, bs, rebalancing_date, what):
        seen[rebalancing_date] = -bs.optimization.objective["scores"]
        append_custom(backtest=backtest, bs=bs, rebalancing_date=rebalancing_date, what=what)

    bs = BacktestService(
        data={"return_series": X, "bm_series": y},
        selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
        optimization_item_builders={
            "return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=WIDTH),
            "bm_series": OptimizationItemBuilder(bibfn=bibfn_bm_series, width=WIDTH),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=1),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, upper=0.1)},
        rebdates=rebdates, append_fun=append_fun, append_fun_args=["w_dict"])
    bs.optimization = PercentilePortfolios(n_percentile=5, estimator=estimator())   # (sic: ignored)
    bt = Backtest()
    bt.run(bs=bs)
    N = 5
    keep, b_scores, b_w, b_masks, b_gap = [], [], [], [], []
    for i, d in enumerate(rebdates):
        s = seen[d]
        assert list(s.index) == names and not (s == 0).any()
        gap = score_gap(-s.to_numpy(), N)
        if gap < MIN_GAP:
            continue
        port = bt.strategy.portfolios[i]
        assert port.rebalancing_date == d
        keep.append(d)
        b_gap.append(gap)
        b_scores.append(s.to_numpy(dtype=np.float64))
        b_w.append([port.weights[k] for k in names])
        b_masks.append([[k in bt.output[d][f"weights_{q}"].index for k in names] for q in range(1, N + 1)])
    dropped = len(rebdates) - len(keep)
    assert dropped <= MAX_DROP * len(rebdates), (dropped, len(rebdates))
    out.update(b_all_rebdates=np.array(rebdates), b_rebdates=np.array(keep), b_dropped=np.int64(dropped),
               b_scores=np.array(b_scores), b_w=np.array(b_w, dtype=np.float64), b_masks=np.array(b_masks),
               b_gap=np.array(b_gap), min_gap=np.float64(min(min(a_gap), min(b_gap))))
    np.savez_compressed(os.path.join(cg.OUT, "msci_percentile.npz"), **out)
    print({k: getattr(v, "shape", v) for k, v in out.items()})
    print(f"dates kept {len(keep)} of {len(rebdates)}; smallest gap {float(out['min_gap']):.3e}")


if __name__ == "__main__":
    main()
