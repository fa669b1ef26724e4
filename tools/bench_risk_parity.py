#!/usr/bin/env python3
"""Risk-parity portfolios (RiskParity, pq_risk_parity_batched) at the config-3 shape: synthetic
5000 x 1000 factor panel, 252-day windows, 4749 daily dates, equal budgets, sample covariance.
One JSON line:

* ``engine_ms``: engine.risk_parity_weights on all dates (window means, diag(Xc'Xc) and the
  coordinate-descent kernel), HIP-event time, median of --reps calls; ``kernel_ms``: the kernel's
  launch alone (means and diagonals precomputed); dates/s from the latter;
* ``sweeps_mean`` / ``sweeps_max`` and the status counts;
* ``traffic_bytes``: the algorithmic traffic sweeps * T * n * 8 B per date (every sweep reads the
  date's window once) and the share of the 8 TB/s HBM peak it implies at ``kernel_ms`` (the
  windows of neighbouring dates overlap, so most of it is served from L2 / the Infinity Cache);
* ``backtest_ms``: Backtest.run (batched, no append_fun), host clock, median of --steps runs
  after one warm-up;
* ``numpy_s_per_date``: the float64 numpy restatement of the blocked recurrence (below) on
  --host-dates dates on the host, for scale.
Experiment tooling; the numbers are quoted in README.md and DESIGN.md."""
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
from porqua_amd import _lib, engine  # noqa: E402
from porqua_amd.backtest import Backtest  # noqa: E402
from porqua_amd.optimization import RiskParity  # noqa: E402
from porqua_amd.synthetic import factor_panel  # noqa: E402

HBM_PEAK = 8.0e12


def risk_parity_numpy(X, b, eps=1e-10, max_sweeps=500, tile=16):
    """The kernel's recurrence in float64 numpy on one T x n window (sample covariance):
    16 assets per step, r = Xc y carried along; the residual after every sweep with r recomputed."""
    T, n = X.shape
    Xc = X - X.mean(axis=0)
    a = 1.0 / (T - 1)
    dg = np.einsum("ti,ti->i", Xc, Xc)
    d = a * dg
    y = np.sqrt(b / d)
    r = Xc @ y
    for k in range(1, max_sweeps + 1):
        for j0 in range(0, n, tile):
            Xt = Xc[:, j0:j0 + tile]
            G = a * (Xt.T @ Xt)
            g = a * (Xt.T @ r)
            delta = np.zeros(Xt.shape[1])
            for i in range(Xt.shape[1]):
                j = j0 + i
                s = g[i] + G[i, :i] @ delta[:i] - d[j] * y[j]
                q = np.sqrt(s * s + 4.0 * d[j] * b[j])
                ynew = 2.0 * b[j] / (s + q) if s > 0 else (q - s) / (2.0 * d[j])
                delta[i] = ynew - y[j]
                y[j] = ynew
            r += Xt @ delta
        r = Xc @ y
        if np.max(np.abs(y * (a * (Xc.T @ r)) - b) / b) <= eps:
            break
    return y / y.sum(), k


def _event_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--dates", type=int, default=4749)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-dates", type=int, default=8)
    a = ap.parse_args()
    width = 252
    dates, R, y, _ = factor_panel(a.days, a.n)
    idx = pd.DatetimeIndex(dates)
    X = pd.DataFrame(R, index=idx, columns=[f"a{i}" for i in range(a.n)])
    Y = pd.DataFrame({"bm": y}, index=idx)
    rebdates = [str(d.date()) for d in idx[width - 1:][:a.dates]]
    B = len(rebdates)

    # ---- the engine call and the kernel alone ---------------------------------------------
    pan = engine.Panel(R)
    rows, tlen = engine.window_rows(dates.astype("datetime64[D]"), np.array(rebdates, dtype="datetime64[D]"), width)
    rd, td = pan.rows_to_device(rows, tlen)
    x, stats, status = engine.risk_parity_weights(pan, rd, td)      # warm-up
    torch.cuda.synchronize()
    engine_ms, _ = _event_ms(lambda: engine.risk_parity_weights(pan, rd, td), a.reps)
    mu = pan.window_means(rd, td)
    dg = pan.window_sumsq(rd, td, mu)
    kernel_ms, kernel_ms_min = _event_ms(lambda: engine.risk_parity_weights(pan, rd, td, moments=(mu, dg)), a.reps)
    st = stats.cpu().numpy()
    code = status.cpu().numpy()
    sweeps = st[:, 1]
    T = int(tlen.max())
    traffic = float(sweeps.sum()) * T * a.n * 8

    # ---- Backtest.run -------------------------------------------------------------------------
    def run():
        bt = Backtest()
        bt.run(service(RiskParity(), X, Y, rebdates, width))
        return bt
    run()
    runs = []
    for _ in range(a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bt = run()
        runs.append(time.perf_counter() - t0)

    # ---- the numpy restatement on the host ----------------------------------------------------
    hd = min(B, a.host_dates)
    b = np.full(a.n, 1.0 / a.n)
    xh = x[:hd].cpu().numpy()
    t0 = time.perf_counter()
    err, ksw = 0.0, []
    for i in range(hd):
        xi, k = risk_parity_numpy(R[rows[i, :tlen[i]]], b)
        err = max(err, float(np.max(np.abs(xi / xh[i] - 1))))
        ksw.append(k)
    host_s = time.perf_counter() - t0
    print(json.dumps({
        "n": a.n, "T": T, "dates": B, "path": bt.stats.get("path"),
        "status_ok": int((code == _lib.PQ_RP_OK).sum()), "status_max_sweeps": int((code == _lib.PQ_RP_MAX_SWEEPS).sum()),
        "status_bad_input": int((code == _lib.PQ_RP_BAD_INPUT).sum()),
        "sweeps_mean": float(sweeps.mean()), "sweeps_max": float(sweeps.max()), "res_max": float(st[:, 0].max()),
        "engine_ms": engine_ms, "kernel_ms": kernel_ms, "kernel_ms_min": kernel_ms_min,
        "dates_per_s": B / (kernel_ms * 1e-3),
        "traffic_bytes": traffic, "traffic_hbm_fraction": traffic / (kernel_ms * 1e-3) / HBM_PEAK,
        "backtest_ms": float(np.median(runs)) * 1e3, "backtest_ms_all": [r * 1e3 for r in runs],
        "backtest_dates_per_s": B / float(np.median(runs)),
        "numpy_s_per_date": host_s / hd, "numpy_dates": hd, "numpy_sweeps": ksw,
        "numpy_vs_device_max_rel": err}), flush=True)


if __name__ == "__main__":
    main()
