#!/usr/bin/env python3
"""The exponentially weighted covariance (engine.ewma_cov, pq_ewma_cov_batched) at the config-3
shape: synthetic 5000 x 1000 factor panel, 252-day windows, 4749 daily dates, chunks of dates whose
dense output fills --chunk-gib (256 dates per 2 GiB).  One JSON line:

* ``ewma_direct_ms`` / ``ewma_slide_ms``: HIP-event times of pq_ewma_cov_batched (the weighted
  moments kernel and the weighted SYRK, or the sliding recursion over the chunk's SlidePlan) into
  preallocated buffers, summed over the chunks, median of --reps passes, every pass in ``*_all``;
* ``pearson_direct_ms`` / ``pearson_slide_ms``: Panel.cov(mode=0) and Panel.cov(mode=0, plan=) --
  window means included -- on the same chunks into the same buffer in the same session: the
  yardsticks, equal-weight kernels with the same bytes to write;
* ``*_hbm_fraction``: the share of the 8 TB/s HBM peak that 8 n^2 bytes written per date imply;
* ``ewma_over_pearson_direct`` / ``ewma_over_pearson_slide``: the ratios of the medians, and
  ``pearson_*_spread``: (max - min) / median of the yardstick's own passes, the run-to-run spread
  a ratio has to be read against;
* ``engine_slide_ms``: engine.ewma_cov(plan=) chunk by chunk (age table upload and allocations
  included);
* ``status_bad_input``, and the largest deviation of both kernels from the longdouble model
  (tests/ewma_model.py), relative to sd_i sd_j, on --host-dates dates.
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
from tests import ewma_model as em  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--dates", type=int, default=4749)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--halflife", type=float, default=63.0)
    ap.add_argument("--host-dates", type=int, default=3)
    ap.add_argument("--chunk-gib", type=float, default=2.0, help="the dense output buffer of a chunk of dates, GiB")
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
    mean = torch.empty((per, ld), dtype=torch.float64, device=dev)
    wsum = torch.empty((per, 2), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    wage_host = engine.ewma_age_weights(tmax, halflife=a.halflife)
    wage = torch.from_numpy(wage_host).to(dev)
    wsqrt = torch.empty_like(wage)
    chunks = [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]
    plans = [engine.SlidePlan(rows[b0:b1], tlen[b0:b1], dev) for b0, b1 in chunks]
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def timed(fn):
        marks = []
        for (b0, b1), plan in zip(chunks, plans):
            e0, e1 = ev(), ev()
            e0.record()
            fn(b0, b1, plan)
            e1.record()
            marks.append((e0, e1))
        torch.cuda.synchronize()
        return sum(m[0].elapsed_time(m[1]) for m in marks)

    def ewma(b0, b1, plan):
        _lib.check(lib.pq_ewma_cov_batched(p(pan.R), pan.R.stride(0), n, p(rd[b0:b1]), p(td[b0:b1]), tmax, b1 - b0,
                                           p(wage), p(wsqrt), p(mean), mean.stride(0), p(wsum), p(buf), ld,
                                           buf.stride(0),
                                           p(status[b0:]), p(plan.gstart) if plan else None,
                                           plan.ngroups if plan else 0, p(plan.shift) if plan else None,
                                           engine._stream()), "pq_ewma_cov_batched")

    passes = {
        "pearson_direct": lambda b0, b1, plan: pan.cov(rd[b0:b1], td[b0:b1], mode=0, out=buf[:b1 - b0]),
        "pearson_slide": lambda b0, b1, plan: pan.cov(rd[b0:b1], td[b0:b1], mode=0, out=buf[:b1 - b0], plan=plan),
        "ewma_direct": lambda b0, b1, plan: ewma(b0, b1, None),
        "ewma_slide": ewma,
        "engine_slide": lambda b0, b1, plan: engine.ewma_cov(pan, rd[b0:b1], td[b0:b1], halflife=a.halflife,
                                                             plan=plan, out=buf[:b1 - b0]),
    }
    for fn in passes.values():   # warm-up
        timed(fn)
    # alternate the passes so that no candidate always runs in the same position
    t = {k: [] for k in passes}
    for _ in range(a.reps):
        for k, fn in passes.items():
            t[k].append(timed(fn))
    written = 8.0 * n * n * B
    res = {"n": n, "T": tmax, "dates": B, "halflife": a.halflife, "chunk_gib": a.chunk_gib, "chunks": len(chunks),
           "dates_per_chunk": per, "slide_groups": sum(pl.ngroups for pl in plans), "reps": a.reps,
           "bytes_written": written}
    for k, v in t.items():
        med = float(np.median(v))
        res[f"{k}_ms"] = med
        res[f"{k}_ms_all"] = [float(x) for x in v]
        res[f"{k}_hbm_fraction"] = written / (med * 1e-3) / HBM_PEAK
    for kind in ("direct", "slide"):
        res[f"ewma_over_pearson_{kind}"] = res[f"ewma_{kind}_ms"] / res[f"pearson_{kind}_ms"]
        v = t[f"pearson_{kind}"]
        res[f"pearson_{kind}_spread"] = float((max(v) - min(v)) / np.median(v))
    timed(ewma)
    res["status_bad_input"] = int((status != _lib.PQ_EWMA_OK).sum().item())

    # ---- the longdouble model on a few dates (the first are an anchor and its followers) --------
    hd = min(B, per, a.host_dates)
    err = {}
    for name, plan in (("direct", None), ("slide", plans[0])):
        b1 = chunks[0][1]
        S = engine.ewma_cov(pan, rd[:b1], td[:b1], halflife=a.halflife, plan=plan)[0][:hd].cpu().numpy()
        worst = 0.0
        for i in range(hd):
            mod = em.ewma(R[rows[i, :tlen[i]]], wage_host)
            worst = max(worst, float((np.abs(S[i, :n, :n] - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
        err[name] = worst
    res["host_dates"], res["host_vs_device_max_rel"] = hd, err
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
