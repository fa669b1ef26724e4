#!/usr/bin/env python3
"""Quantile portfolios (PercentilePortfolios, src/optimization.py:356-417) at the config-3
shape: synthetic 5000 x 1000 panel, 252-day windows, 4749 daily dates, n_mom=252, n_rev=21,
quintiles.  Three numbers, one JSON line:

* ``kernel_us``: pq_percentile_batched alone on a (dates x n) score panel, HIP-event time,
  median of --reps launches, and the share of the 8 TB/s HBM peak its algorithmic bytes
  (8 n read + 12 n written per date) imply;
* ``backtest_s``: Backtest.run (batched, no append_fun), host clock around a run that ends in
  a device-to-host copy, median of --steps runs after one warm-up;
* ``host_loop_s``: the reference's work per date on the host (pandas window slice, geometric
  mean, np.percentile, N masks, long-short weights), the same dates in a serial loop.
Experiment tooling; the numbers are quoted in DESIGN.md."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_wls import service  # noqa: E402
from porqua_amd import engine  # noqa: E402
from porqua_amd.backtest import Backtest  # noqa: E402
from porqua_amd.mean_estimation import MeanEstimator  # noqa: E402
from porqua_amd.optimization import PercentilePortfolios  # noqa: E402
from porqua_amd.synthetic import factor_panel  # noqa: E402

HBM_PEAK = 8.0e12


def host_loop(X, ends, width, n_mom, n_rev, N):
    q_vec = np.linspace(0, 100, N + 1)
    W = np.zeros((len(ends), X.shape[1]))
    for k, e in enumerate(ends):
        win = X.iloc[max(0, e - width):e]
        sub = win.tail(n_mom).head(n_mom - n_rev)
        x = -(np.exp(np.log(1 + sub).mean(axis=0)) - 1).to_numpy()
        th = np.percentile(x, q_vec)
        masks = [x <= th[1]] + [np.logical_and(x > th[i - 1], x <= th[i]) for i in range(2, N + 1)]
        w = x * 0
        w[masks[0]] = 1 / masks[0].sum()
        w[masks[-1]] = -1 / masks[-1].sum()
        W[k] = w
    return W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--dates", type=int, default=4749)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-dates", type=int, default=0, help="dates of the host loop (0: all)")
    a = ap.parse_args()
    width, n_mom, n_rev, N = 252, 252, 21, 5
    dates, R, y, _ = factor_panel(a.days, a.n)
    idx = pd.DatetimeIndex(dates)
    X = pd.DataFrame(R, index=idx, columns=[f"a{i}" for i in range(a.n)])
    Y = pd.DataFrame({"bm": y}, index=idx)
    rebdates = [str(d.date()) for d in idx[width - 1:][:a.dates]]
    B = len(rebdates)

    # ---- the kernel alone ---------------------------------------------------------------
    dev = engine.default_device()
    S = torch.from_numpy(0.01 * np.random.default_rng(1).standard_normal((B, a.n))).to(dev)
    for _ in range(10):
        engine.percentile_weights(S, N)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        engine.percentile_weights(S, N)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3)
    kernel_us = float(np.median(times))
    nbytes = B * a.n * 20

    # ---- Backtest.run ---------------------------------------------------------------------
    me = MeanEstimator(method="geometric", n_mom=n_mom, n_rev=n_rev)

    def run():
        bt = Backtest()
        bt.run(service(PercentilePortfolios(estimator=me, n_percentiles=N), X, Y, rebdates, width))
        return bt
    run()
    runs = []
    for _ in range(a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bt = run()
        runs.append(time.perf_counter() - t0)
    W = np.array([list(p.weights.values()) for p in bt.strategy.portfolios])

    # ---- the reference's per-date work on the host -------------------------------------------
    hd = B if a.host_dates <= 0 else min(B, a.host_dates)
    ends = np.arange(width, width + B)[:hd]
    t0 = time.perf_counter()
    Wh = host_loop(X, ends, width, n_mom, n_rev, N)
    host_s = time.perf_counter() - t0
    print(json.dumps({"n": a.n, "dates": B, "n_percentiles": N, "path": bt.stats.get("path"),
                      "kernel_us": kernel_us, "kernel_us_min": float(np.min(times)),
                      "kernel_bytes": nbytes, "kernel_hbm_fraction": nbytes / (kernel_us * 1e-6) / HBM_PEAK,
                      "backtest_s": float(np.median(runs)), "backtest_s_all": runs,
                      "host_loop_s": host_s, "host_loop_dates": hd,
                      "host_loop_s_all_dates": host_s * B / hd,
                      "weights_equal_host_loop": float(np.mean(np.all(W[:hd] == Wh, axis=1)))}), flush=True)


if __name__ == "__main__":
    main()
