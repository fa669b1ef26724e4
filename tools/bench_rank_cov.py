#!/usr/bin/env python3
"""The rank covariances (engine.rank_cov, pq_rank_cov_batched) at the config-3 shape: synthetic
5000 x 1000 factor panel, 252-day windows, 4749 daily dates.  One JSON line:

* ``spearman``: ``rank_ms`` (the ranking kernel), ``gram_ms`` (Panel.cov(mode=1) on the rank panel)
  and ``finish_ms`` (the epilogue kernel); ``kendall``: ``rank_ms`` and ``gram_ms`` (the int8-MFMA
  Gram over day pairs, epilogue included) -- HIP-event times of the stages launched apart (the
  ``stages`` argument of the entry point) on chunks of dates, summed over the chunks, median of
  --reps passes; ``moments_ms``: the window means and sums of squares both start from;
* ``kendall.int8_floor_ms``: (computed 64 x 64 tiles) x 64^2 x T (T - 1) / 2 MACs per date over the
  dense int8 MFMA peak, and ``kendall.gram_over_floor``; ``kendall.steps``: the MFMA k-blocks a
  tile walks against the ceil(T (T - 1) / 2 / 64) of a dense pair list;
* ``pearson_ms``: Panel.cov(mode=0) and ``gerber_ms``: engine.gerber_cov (variant 2, moments
  included) on the same chunks into the same buffer in the same session;
* ``engine_ms`` per kind: engine.rank_cov chunk by chunk, moments included;
* ``status_bad_input``, and whether the counts equal the NumPy model's (tests/rank_model.py) with
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
from tests import rank_model as rm  # noqa: E402

I8_PEAK_MACS = 5.0e15 / 2   # dense int8 MFMA peak (twice BF16's ~2.5 PF per clock: ~5 POPS), in multiply-accumulates / s


def kendall_steps(T):
    """k-blocks of 64 pairs a tile walks: s in blocks of 16, t in blocks of 4 from the block of s."""
    return sum(len(range(s0, T, 4)) for s0 in range(0, T - 1, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--dates", type=int, default=4749)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-dates", type=int, default=1)
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
    scratch = {"spearman": torch.empty((per * tmax, n), dtype=torch.float64, device=dev),
               "kendall": torch.empty((per, ld * engine.round_up(tmax, 64)), dtype=torch.int16, device=dev)}
    ranks = engine.Panel(scratch["spearman"], device=dev)
    rrows = torch.arange(per * tmax, dtype=torch.int32, device=dev).view(per, tmax)
    rlen = torch.full((per,), tmax, dtype=torch.int32, device=dev)
    diag = torch.empty((B, ld), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def rank_pass(kind):
        kd = engine.RANK_KINDS[kind]
        marks = []
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            r, t = rd[b0:b1], td[b0:b1]
            e = [ev() for _ in range(5)]
            e[0].record()
            dg = pan.window_sumsq(r, t, pan.window_means(r, t))
            e[1].record()

            def call(stages):
                _lib.check(lib.pq_rank_cov_batched(p(pan.R), pan.R.stride(0), n, p(r), p(t), tmax, b1 - b0, p(dg),
                                                   dg.stride(0), kd, _lib.PQ_RANK_COV, stages, p(scratch[kind]), n,
                                                   p(diag[b0:]), diag.stride(0), p(buf), ld, buf.stride(0),
                                                   p(status[b0:]), engine._stream()), "pq_rank_cov_batched")
            call(_lib.PQ_RANK_RANKS)
            e[2].record()
            if kind == "spearman":
                ranks.cov(rrows[:b1 - b0], rlen[:b1 - b0], mode=1, out=buf[:b1 - b0])
            e[3].record()
            call(_lib.PQ_RANK_FINISH)
            e[4].record()
            marks.append(e)
        torch.cuda.synchronize()
        return [sum(m[i].elapsed_time(m[i + 1]) for m in marks) for i in range(4)]

    def timed(fn):
        def run():
            e0, e1 = ev(), ev()
            e0.record()
            for b0 in range(0, B, per):
                b1 = min(B, b0 + per)
                fn(rd[b0:b1], td[b0:b1], buf[:b1 - b0])
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    passes = {"pearson": timed(lambda r, t, o: pan.cov(r, t, mode=0, out=o)),
              "gerber": timed(lambda r, t, o: engine.gerber_cov(pan, r, t, out=o)),
              "engine_spearman": timed(lambda r, t, o: engine.rank_cov(pan, r, t, kind="spearman", out=o)),
              "engine_kendall": timed(lambda r, t, o: engine.rank_cov(pan, r, t, kind="kendall", out=o))}
    rank_pass("spearman"), rank_pass("kendall")      # warm-up
    for f in passes.values():
        f()
    res = {"n": n, "T": tmax, "dates": B, "chunk_gib": a.chunk_gib, "chunks": -(-B // per), "dates_per_chunk": per}
    # alternate the passes so that no candidate always runs in the same position
    t = {k: [] for k in ("spearman", "kendall", *passes)}
    for _ in range(a.reps):
        for k, f in passes.items():
            t[k].append(f())
        t["spearman"].append(rank_pass("spearman"))
        t["kendall"].append(rank_pass("kendall"))
    for kind in ("spearman", "kendall"):
        m = np.median(np.array(t[kind]), axis=0)
        res[kind] = {"moments_ms": float(m[0]), "rank_ms": float(m[1])}
        if kind == "spearman":
            res[kind].update(gram_ms=float(m[2]), finish_ms=float(m[3]), kernels_ms=float(m[1] + m[2] + m[3]))
        else:
            res[kind].update(gram_ms=float(m[3]), kernels_ms=float(m[1] + m[3]))
        res[kind]["kernels_ms_all"] = [float(sum(x[1:])) for x in t[kind]]
        res[kind]["engine_ms"] = float(np.median(t["engine_" + kind]))
    nt = ld // 64
    tiles = nt * (nt + 1) // 2
    floor = tiles * 64 * 64 * (tmax * (tmax - 1) // 2) * B / I8_PEAK_MACS * 1e3
    res["kendall"].update(tiles_per_date=tiles, int8_floor_ms=floor, gram_over_floor=res["kendall"]["gram_ms"] / floor,
                          steps=kendall_steps(tmax), dense_steps=-(-(tmax * (tmax - 1) // 2) // 64))
    res["pearson_ms"] = float(np.median(t["pearson"]))
    res["pearson_ms_all"] = [float(x) for x in t["pearson"]]
    res["gerber_ms"] = float(np.median(t["gerber"]))
    res["spearman_over_pearson"] = res["spearman"]["engine_ms"] / res["pearson_ms"]
    res["status_bad_input"] = int((status != _lib.PQ_RANK_OK).sum().item())

    # ---- the NumPy model on a few dates ---------------------------------------------------------
    hd = min(B, a.host_dates)
    err, same = 0.0, True
    for kind in ("spearman", "kendall"):
        N = engine.rank_cov(pan, rd[:hd], td[:hd], kind=kind, output="counts")[0].cpu().numpy()
        S = engine.rank_cov(pan, rd[:hd], td[:hd], kind=kind)[0].cpu().numpy()
        for i in range(hd):
            mod = rm.rank_cov(R[rows[i, :tlen[i]]], kind)
            same = same and bool(np.array_equal(N[i, :n, :n], mod.counts))
            err = max(err, float((np.abs(S[i, :n, :n] - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
    res["host_dates"], res["host_counts_equal"], res["host_vs_device_max_rel"] = hd, same, err
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
