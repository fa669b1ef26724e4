#!/usr/bin/env python3
"""Hierarchical risk parity (HierarchicalRiskParity, pq_hrp_batched) at the config-3 shape:
synthetic 5000 x 1000 factor panel, 252-day windows, 4749 daily dates, sample covariance (singular:
more assets than window rows).  One JSON line:

* ``engine_ms``: engine.hrp_weights on all dates (the dense covariance of every chunk of dates and
  one kernel launch per chunk), HIP-event time, median of --reps calls;
* ``cov_ms`` / ``kernel_ms``: the same chunks with events between the covariance formation
  (Panel.cov) and the HRP kernel, summed over the chunks, median of --reps passes; dates/s from
  ``kernel_ms``;
* ``traffic_bytes``: the algorithmic traffic per date and the share of the 8 TB/s HBM peak it
  implies at ``kernel_ms``.  'single': 2 x 8 n^2 B (Prim reads every row once, the bisection's two
  passes over the cross blocks half the matrix each).  The chain methods (--method complete,
  average, weighted, ward): 8 n^2 to read S and 8 n^2 to write D (the fill), a row of 8 n per scan
  with at most 3 n scans, per merge one more row read, the new row and the new column written
  (3 x 8 n, n merges), and the bisection's 8 n^2: 72 n^2 B, an upper bound (the strided column
  writes cost the memory system whole lines).  --chunk-gib sets the dense buffer, hence the dates
  (one workgroup each) a launch has to fill the CUs with; the chain methods hold a second buffer
  of that size;
* ``min_gap_min``: the smallest reported gap between consecutive merge distances over the dates;
* ``backtest_ms``: Backtest.run (batched, no append_fun), host clock, median of --steps runs after
  one warm-up (null for 'ward', which HierarchicalRiskParity does not open);
* ``host_s_per_date``: NumPy + SciPy (linkage with the same method, leaves_list, the recursive bisection) on
  --host-dates dates on the host, for scale, with the largest relative weight difference from the
  device and whether the leaf orders agree.
Experiment tooling; the numbers are quoted in README.md and DESIGN.md."""
import argparse
import ctypes
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
from porqua_amd.optimization import HRP_LINKAGES, HierarchicalRiskParity  # noqa: E402
from porqua_amd.synthetic import factor_panel  # noqa: E402

HBM_PEAK = 8.0e12


def hrp_scipy(X, method="single"):
    """HRP of one T x n window on the host: SciPy's linkage, then the bisection in numpy."""
    from scipy.cluster.hierarchy import leaves_list, linkage
    from scipy.spatial.distance import squareform
    S = np.cov(X.T)
    sd = np.sqrt(np.diag(S))
    D = np.sqrt(np.clip(1.0 - S / np.outer(sd, sd), 0.0, 2.0) / 2.0)
    np.fill_diagonal(D, 0.0)
    order = leaves_list(linkage(squareform(D, checks=False), method))
    w = np.ones(len(order))
    lists = [order]

    def cvar(idx):
        Sc = S[np.ix_(idx, idx)]
        u = 1.0 / np.diag(Sc)
        u /= u.sum()
        return u @ Sc @ u
    while lists:
        nxt = []
        for c in lists:
            if len(c) < 2:
                continue
            left, right = c[:len(c) // 2], c[len(c) // 2:]
            vl, vr = cvar(left), cvar(right)
            al = 1.0 - vl / (vl + vr)
            w[left] *= al
            w[right] *= 1.0 - al
            nxt += [left, right]
        lists = nxt
    return w, order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--dates", type=int, default=4749)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-dates", type=int, default=4)
    ap.add_argument("--chunk-gib", type=float, default=engine.HRP_CHUNK_BYTES / 2 ** 30,
                    help="the dense covariance buffer (engine.hrp_weights' chunk_bytes), GiB")
    ap.add_argument("--method", choices=list(_lib.HRP_METHODS), default="single", help="the linkage of the tree")
    a = ap.parse_args()
    chunk_bytes = int(a.chunk_gib * 2 ** 30)
    width = 252
    dates, R, y, _ = factor_panel(a.days, a.n)
    idx = pd.DatetimeIndex(dates)
    X = pd.DataFrame(R, index=idx, columns=[f"a{i}" for i in range(a.n)])
    Y = pd.DataFrame({"bm": y}, index=idx)
    rebdates = [str(d.date()) for d in idx[width - 1:][:a.dates]]
    B, n = len(rebdates), a.n

    pan = engine.Panel(R)
    rows, tlen = engine.window_rows(dates.astype("datetime64[D]"), np.array(rebdates, dtype="datetime64[D]"), width)
    rd, td = pan.rows_to_device(rows, tlen)
    x, order, stats, status = engine.hrp_weights(pan, rd, td, chunk_bytes=chunk_bytes, method=a.method)       # warm-up
    torch.cuda.synchronize()

    def ev():
        return torch.cuda.Event(enable_timing=True)
    eng = []
    for _ in range(a.reps):
        t0, t1 = ev(), ev()
        t0.record()
        engine.hrp_weights(pan, rd, td, chunk_bytes=chunk_bytes, method=a.method)
        t1.record()
        t1.synchronize()
        eng.append(t0.elapsed_time(t1))

    # ---- the same chunks, covariance and kernel timed apart ---------------------------------
    lib = _lib.load()
    ld = engine.round_up(n, 64)
    per = max(1, min(B, chunk_bytes // (8 * ld * ld)))
    buf = torch.empty((per, ld, ld), dtype=torch.float64, device=pan.device)
    meth = _lib.HRP_METHODS[a.method]
    work = torch.empty((per, n, ld), dtype=torch.float64, device=pan.device) if meth != _lib.PQ_HRP_SINGLE else None
    one = torch.ones(B, dtype=torch.float64, device=pan.device)
    zero = torch.zeros(B, dtype=torch.float64, device=pan.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    covs, kers = [], []
    for _ in range(a.reps):
        marks = []
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            S = pan.cov(rd[b0:b1], td[b0:b1], out=buf[:b1 - b0])
            e1.record()
            _lib.check(lib.pq_hrp_linkage_batched(p(S), ld, n, b1 - b0, p(one[b0:]), p(zero[b0:]), 1.0, meth,
                                                  None if work is None else p(work), ld, p(x[b0:]), x.stride(0),
                                                  p(order[b0:]), order.stride(0), None, p(stats[b0:]),
                                                  p(status[b0:]), None), "pq_hrp_linkage_batched")
            e2.record()
            marks.append((e0, e1, e2))
        torch.cuda.synchronize()
        covs.append(sum(m[0].elapsed_time(m[1]) for m in marks))
        kers.append(sum(m[1].elapsed_time(m[2]) for m in marks))
    cov_ms, kernel_ms = float(np.median(covs)), float(np.median(kers))
    st = stats.cpu().numpy()
    code = status.cpu().numpy()
    traffic = (2.0 if meth == _lib.PQ_HRP_SINGLE else 9.0) * 8.0 * n * n * B

    # ---- Backtest.run -------------------------------------------------------------------------
    def run():
        bt = Backtest()
        bt.run(service(HierarchicalRiskParity(linkage=a.method), X, Y, rebdates, width))
        return bt
    runs, bt = [], None
    if a.method in HRP_LINKAGES:   # (Ward is reachable through engine.hrp_weights alone)
        run()
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bt = run()
            runs.append(time.perf_counter() - t0)

    # ---- NumPy + SciPy on the host ----------------------------------------------------------------
    hd = min(B, a.host_dates)
    xh, oh = x[:hd].cpu().numpy(), order[:hd].cpu().numpy()
    t0 = time.perf_counter()
    err, same = 0.0, True
    for i in range(hd):
        wi, oi = hrp_scipy(R[rows[i, :tlen[i]]], a.method)
        err = max(err, float(np.max(np.abs(wi / xh[i] - 1))))
        same = same and bool(np.array_equal(oi, oh[i]))
    host_s = time.perf_counter() - t0
    print(json.dumps({
        "method": a.method, "n": n, "T": int(tlen.max()), "dates": B, "chunk_gib": a.chunk_gib, "chunks": -(-B // per), "dates_per_chunk": per,
        "path": bt.stats.get("path") if bt else None,
        "status_ok": int((code == _lib.PQ_HRP_OK).sum()), "status_bad_input": int((code == _lib.PQ_HRP_BAD_INPUT).sum()),
        "min_gap_min": float(st[:, 1].min()), "sum_x_max_dev": float((x.sum(dim=1) - 1).abs().max()),
        "engine_ms": float(np.median(eng)), "cov_ms": cov_ms, "kernel_ms": kernel_ms, "kernel_ms_min": float(np.min(kers)),
        "kernel_us_per_date": kernel_ms * 1e3 / B, "dates_per_s": B / (kernel_ms * 1e-3),
        "traffic_bytes": traffic, "traffic_hbm_fraction": traffic / (kernel_ms * 1e-3) / HBM_PEAK,
        "backtest_ms": float(np.median(runs)) * 1e3 if runs else None, "backtest_ms_all": [r * 1e3 for r in runs],
        "backtest_dates_per_s": B / float(np.median(runs)) if runs else None,
        "host_s_per_date": host_s / hd, "host_dates": hd, "host_vs_device_max_rel": err,
        "host_order_equal": same}), flush=True)


if __name__ == "__main__":
    main()
