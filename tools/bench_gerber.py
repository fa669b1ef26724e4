#!/usr/bin/env python3
"""The Gerber covariance (engine.gerber_cov, pq_gerber_cov_batched) at the config-3 shape: synthetic
5000 x 1000 factor panel, 252-day windows, 4749 daily dates.  One JSON line:

* per variant (``v1`` / ``v2``) ``sign_ms`` and ``gram_ms``: HIP-event times of the sign kernel and
  of the int8-MFMA Gram kernel, launched apart (the ``stages`` argument of the entry point) on
  chunks of dates whose dense output fills --chunk-gib, summed over the chunks, median of --reps
  passes; ``moments_ms``: the window means and sums of squares both variants start from;
* ``hbm_fraction``: the share of the 8 TB/s HBM peak that 8 n^2 bytes written per date imply at
  ``sign_ms + gram_ms``;
* ``pearson_ms``: Panel.cov(mode=0), the sample covariance, on the same chunks into the same buffer
  in the same session (window means included) -- the yardstick: the Gerber kernels have less to
  read and the same bytes to write;
* ``engine_ms``: engine.gerber_cov (variant 2) chunk by chunk, moments included;
* ``status_bad_input``, and whether the counts equal the NumPy model's (tests/gerber_model.py) with
  the largest deviation of Sigma from it, relative to sd_i sd_j, on --host-dates dates.
Experiment tooling; the numbers are quoted in README.md and DESIGN.md."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from porqua_amd import _lib, engine  # noqa: E402
from porqua_amd.synthetic import factor_panel  # noqa: E402
from tests import gerber_model as gm  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--dates", type=int, default=4749)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--host-dates", type=int, default=2)
    ap.add_argument("--chunk-gib", type=float, default=engine.HRP_CHUNK_BYTES / 2 ** 30,
                    help="the dense output buffer of a chunk of dates, GiB")
    a = ap.parse_args()
    width = 252
    dates, R, _, _ = factor_panel(a.days, a.n)
    reb = dates.astype("datetime64[D]")[width - 1:][:a.dates]
    B, n = len(reb), a.n
    pan = engine.Panel(R)
    rows, tlen = engine.window_rows(dates.astype("datetime64[D]"), reb, width)
    rd, td = pan.rows_to_device(rows, tlen)
    tmax = int(rd.shape[1])
    lib = _lib.load()
    ld = engine.round_up(n, 64)
    per = max(1, min(B, int(a.chunk_gib * 2 ** 30) // (8 * ld * ld)))
    dev = pan.device
    buf = torch.zeros((per, ld, ld), dtype=torch.float64, device=dev)
    St = torch.empty((per, ld * engine.round_up(tmax, 64)), dtype=torch.int8, device=dev)
    counts = torch.empty((B, ld), dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def gerber_pass(variant):
        marks = []
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            r, t = rd[b0:b1], td[b0:b1]
            e = [ev() for _ in range(4)]
            e[0].record()
            dg = pan.window_sumsq(r, t, pan.window_means(r, t))
            e[1].record()
            for k, stage in enumerate((_lib.PQ_GERBER_SIGNS, _lib.PQ_GERBER_GRAM)):
                _lib.check(lib.pq_gerber_cov_batched(p(pan.R), pan.R.stride(0), n, p(r), p(t), tmax, b1 - b0, p(dg),
                                                     dg.stride(0), a.threshold, variant, 0, stage, p(St), p(counts[b0:]),
                                                     counts.stride(0), p(buf), ld, buf.stride(0), p(status[b0:]),
                                                     engine._stream()), "pq_gerber_cov_batched")
                e[2 + k].record()
            marks.append(e)
        torch.cuda.synchronize()
        return [sum(m[i].elapsed_time(m[i + 1]) for m in marks) for i in range(3)]

    def pearson_pass():
        marks = []
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            e0, e1 = ev(), ev()
            e0.record()
            pan.cov(rd[b0:b1], td[b0:b1], mode=0, out=buf[:b1 - b0])
            e1.record()
            marks.append((e0, e1))
        torch.cuda.synchronize()
        return sum(m[0].elapsed_time(m[1]) for m in marks)

    def engine_pass():
        e0, e1 = ev(), ev()
        e0.record()
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            engine.gerber_cov(pan, rd[b0:b1], td[b0:b1], threshold=a.threshold, out=buf[:b1 - b0])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    gerber_pass(2), gerber_pass(1), pearson_pass(), engine_pass()      # warm-up
    res = {"n": n, "T": tmax, "dates": B, "threshold": a.threshold, "chunk_gib": a.chunk_gib, "chunks": -(-B // per),
           "dates_per_chunk": per}
    written = 8.0 * n * n * B
    # alternate the passes so that no candidate always runs in the same position
    t = {1: [], 2: [], "pearson": [], "engine": []}
    for _ in range(a.reps):
        t["pearson"].append(pearson_pass())
        t[2].append(gerber_pass(2))
        t[1].append(gerber_pass(1))
        t["engine"].append(engine_pass())
    for v in (1, 2):
        m = np.median(np.array(t[v]), axis=0)
        res[f"v{v}"] = {"moments_ms": float(m[0]), "sign_ms": float(m[1]), "gram_ms": float(m[2]),
                        "kernels_ms": float(m[1] + m[2]),
                        "kernels_ms_all": [float(x[1] + x[2]) for x in t[v]],
                        "hbm_fraction": written / ((m[1] + m[2]) * 1e-3) / HBM_PEAK}
    res["pearson_ms"] = float(np.median(t["pearson"]))
    res["pearson_ms_all"] = [float(x) for x in t["pearson"]]
    res["engine_ms"] = float(np.median(t["engine"]))
    res["bytes_written"] = written
    res["status_bad_input"] = int((status != _lib.PQ_GERBER_OK).sum().item())

    # ---- the NumPy model on a few dates ---------------------------------------------------------
    hd = min(B, a.host_dates)
    err, same = 0.0, True
    for variant in (1, 2):
        S, st, cnt = engine.gerber_cov(pan, rd[:hd], td[:hd], threshold=a.threshold, variant=variant)
        Sh, cn = S.cpu().numpy(), cnt.cpu().numpy()
        for i in range(hd):
            mod = gm.gerber(R[rows[i, :tlen[i]]], a.threshold, variant)
            same = same and bool(np.array_equal(cn[i, :n], mod.a))
            err = max(err, float((np.abs(Sh[i, :n, :n] - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
    res["host_dates"], res["host_counts_equal"], res["host_vs_device_max_rel"] = hd, same, err
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
