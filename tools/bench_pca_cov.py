#!/usr/bin/env python3
"""The PCA factor covariance (engine.pca_window_form, Covariance 'pca') at the config-3 shape:
synthetic 5000 x 1000 factor panel, 252-day windows, 4749 daily dates.  One JSON line per
``--n-factors`` value ('mp' and 12 by default):

* ``gram_ms`` / ``project_ms``: HIP-event times of pq_window_gram_batched and
  pq_window_project_batched summed over the chunks, median of --reps passes, with the share of the
  8 TB/s HBM peak of their algorithmic traffic (Gram: the window read once, 8 T n, and G written,
  8 ldg^2; projection: the window and the k eigenvector columns read, the k factor rows written);
* ``eig_jacobi_ms`` / ``eig_rocsolver_ms``: helper_functions.sym_eig and torch.linalg.eigh on the
  same Grams (both synchronise inside; the events bracket the whole call);
* ``map_ms``: the eigenvalue map (sort, cumulative sums, sigma2, the factor count) in torch;
* ``form_ms``: engine.pca_window_form end to end for each backend;
* ``rp_factor_ms`` / ``rp_pearson_ms``: pq_risk_parity_batched (engine.risk_parity_weights with the
  moments precomputed) on the factor form and on the sample covariance, sweeps alongside;
* ``hrp_factor_*`` / ``hrp_pearson_*``: the covariance formation and the HRP kernel of
  engine.hrp_weights' chunks on the factor form (the Gram of k rows) and on the sample covariance.
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
from porqua_amd.helper_functions import sym_eig  # noqa: E402
from porqua_amd.synthetic import factor_panel  # noqa: E402

HBM_PEAK = 8.0e12
F64 = torch.float64


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn):
    t0, t1 = ev(), ev()
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def stages(pan, rd, td, nf, kmax, chunk_bytes):
    """One pass over the chunks of pca_window_form with events around every stage."""
    lib = _lib.load()
    B, tmax = rd.shape
    n, dev = pan.n, pan.device
    ldg = engine.round_up(tmax, 64)
    work = int(lib.pq_sym_eig_work_doubles(ldg))
    per = max(1, min(B, chunk_bytes // (8 * (2 * ldg * ldg + work))))
    mp = nf == "mp"
    kcap = min(kmax, n - 1) if mp else int(nf)
    t = dict(moments=0.0, gram=0.0, jacobi=0.0, rocsolver=0.0, map=0.0, project=0.0)
    ktot, unconv = 0, 0
    G = torch.empty((per, ldg, ldg), dtype=F64, device=dev)
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        r, tl = rd[b0:b1], td[b0:b1]
        nb = b1 - b0
        dt, (mu, dg) = timed(lambda: (lambda m: (m, pan.window_sumsq(r, tl, m)))(pan.window_means(r, tl)))
        t["moments"] += dt
        Gc = G[:nb]
        dt, _ = timed(lambda: _lib.check(lib.pq_window_gram_batched(
            p(pan.R), pan.R.stride(0), n, p(r), p(tl), tmax, nb, p(mu), mu.stride(0), p(Gc), ldg, ldg * ldg,
            engine._stream()), "pq_window_gram_batched"))
        t["gram"] += dt
        dt, _ = timed(lambda: torch.linalg.eigh(Gc[:, :tmax, :tmax]))
        t["rocsolver"] += dt
        dt, (evals, V) = timed(lambda: sym_eig(Gc, tmax))
        t["jacobi"] += dt
        unconv += sym_eig.last_unconverged
        fin = torch.ones(nb, dtype=torch.bool, device=dev)
        dt, (kc, sig, lk, s, col, _) = timed(lambda: engine._pca_eigen_map(evals[:, :tmax], dg[:, :n], tl, n, kcap,
                                                                          mp, fin))
        t["map"] += dt
        fr = (torch.cumsum(kc, 0, dtype=torch.int64) - kc).to(torch.int32)
        total = int(kc.sum().item())
        ktot += total
        F = torch.empty((max(total, 1), n), dtype=F64, device=dev)
        dt, _ = timed(lambda: _lib.check(lib.pq_window_project_batched(
            p(pan.R), pan.R.stride(0), n, p(r), p(tl), tmax, nb, p(mu), mu.stride(0), p(V), ldg, ldg * ldg, p(col),
            p(s), p(kc), kcap, p(fr), p(F), n, engine._stream()), "pq_window_project_batched"))
        t["project"] += dt
        del V, evals, F
    return t, ktot, unconv, per


def hrp_split(pan, rd, td, alpha, c, centred, chunk_bytes=engine.HRP_CHUNK_BYTES):
    """(cov ms, kernel ms) of engine.hrp_weights' chunks, single linkage."""
    lib = _lib.load()
    B, n, dev = rd.shape[0], pan.n, pan.device
    ld = engine.round_up(n, 64)
    per = max(1, min(B, chunk_bytes // (8 * ld * ld)))
    buf = torch.empty((per, ld, ld), dtype=F64, device=dev)
    x = torch.empty((B, n), dtype=F64, device=dev)
    order = torch.empty((B, n), dtype=torch.int32, device=dev)
    stats = torch.empty((B, 2), dtype=F64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    tc = tk = 0.0
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        dt, S = timed(lambda: pan.cov(rd[b0:b1], td[b0:b1], mode=0 if centred else 1, out=buf[:b1 - b0]))
        tc += dt
        dt, _ = timed(lambda: _lib.check(lib.pq_hrp_linkage_batched(
            p(S), ld, n, b1 - b0, p(alpha[b0:]), p(c[b0:]), 1.0, _lib.PQ_HRP_SINGLE, None, ld, p(x[b0:]), x.stride(0),
            p(order[b0:]), order.stride(0), None, p(stats[b0:]), p(status[b0:]), engine._stream()),
            "pq_hrp_linkage_batched"))
        tk += dt
    return tc, tk, int((status == _lib.PQ_HRP_OK).sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--dates", type=int, default=4749)
    ap.add_argument("--width", type=int, default=252)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kmax", type=int, default=64)
    ap.add_argument("--n-factors", nargs="+", default=["mp", "12"])
    ap.add_argument("--chunk-gib", type=float, default=engine.PCA_CHUNK_BYTES / 2 ** 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pca_cov needs a GPU"
    chunk_bytes = int(a.chunk_gib * 2 ** 30)
    dates, R, _, _ = factor_panel(a.days, a.n)
    reb = dates[a.width - 1:][:a.dates]
    pan = engine.Panel(R)
    rows, tlen = engine.window_rows(dates.astype("datetime64[D]"), reb.astype("datetime64[D]"), a.width)
    rd, td = pan.rows_to_device(rows, tlen)
    B, n, T = len(reb), a.n, int(tlen.max())
    ldg = engine.round_up(T, 64)
    med = lambda v: float(np.median(v))   # noqa: E731

    # ---- pearson: the risk-parity and HRP kernels on the T-row window form, this session ----
    mu = pan.window_means(rd, td)
    dg = pan.window_sumsq(rd, td, mu)
    rp = lambda: engine.risk_parity_weights(pan, rd, td, moments=(mu, dg))   # noqa: E731
    rp()
    rp_p = [timed(rp) for _ in range(a.reps)]
    sw_p = rp_p[-1][1][1][:, 1]
    one = torch.ones(B, dtype=F64, device=pan.device)
    zero = torch.zeros(B, dtype=F64, device=pan.device)
    hrp_split(pan, rd, td, one, zero, True)
    hp = [hrp_split(pan, rd, td, one, zero, True) for _ in range(a.reps)]
    base = {"rp_pearson_ms": med([v[0] for v in rp_p]), "rp_pearson_sweeps_mean": float(sw_p.mean()),
            "hrp_pearson_cov_ms": med([v[0] for v in hp]), "hrp_pearson_kernel_ms": med([v[1] for v in hp])}

    for nf in a.n_factors:
        nf = nf if nf == "mp" else int(nf)
        stages(pan, rd, td, nf, a.kmax, chunk_bytes)                                     # warm-up
        runs = [stages(pan, rd, td, nf, a.kmax, chunk_bytes) for _ in range(a.reps)]
        t = {k: med([r[0][k] for r in runs]) for k in runs[0][0]}
        ktot, unconv, per = runs[0][1:]
        form = {}
        for backend in ("jacobi", "rocsolver"):
            engine.pca_window_form(pan, rd, td, nf, backend=backend, kmax=a.kmax, chunk_bytes=chunk_bytes)
            form[backend] = med([timed(lambda: engine.pca_window_form(pan, rd, td, nf, backend=backend, kmax=a.kmax,
                                                                      chunk_bytes=chunk_bytes))[0]
                                 for _ in range(a.reps)])
        pf = engine.pca_window_form(pan, rd, td, nf, kmax=a.kmax, chunk_bytes=chunk_bytes)
        k_h = pf.tlen.cpu().numpy()
        dgf = pf.panel.window_sumsq(pf.rows, pf.tlen, None)
        rpf = lambda: engine.risk_parity_weights(pf.panel, pf.rows, pf.tlen, a=1.0, c=pf.sigma2, centred=False,   # noqa: E731
                                                 moments=(None, dgf))
        rpf()
        rp_f = [timed(rpf) for _ in range(a.reps)]
        st_f = rp_f[-1][1]
        hrp_split(pf.panel, pf.rows, pf.tlen, one, pf.sigma2, False)
        hf = [hrp_split(pf.panel, pf.rows, pf.tlen, one, pf.sigma2, False) for _ in range(a.reps)]
        gram_bytes = B * 8.0 * (T * n + ldg * ldg)
        proj_bytes = 8.0 * (B * T * n + ktot * T + ktot * n)
        print(json.dumps({
            "n_factors": nf, "n": n, "T": T, "dates": B, "kmax": a.kmax, "chunks": -(-B // per), "dates_per_chunk": per,
            "k_min": int(k_h.min()), "k_max": int(k_h.max()), "k_mean": float(k_h.mean()),
            "status_ok": int((pf.status == _lib.PQ_PCA_OK).sum().item()), "factor_rows": ktot,
            "moments_ms": t["moments"], "gram_ms": t["gram"], "gram_hbm_fraction": gram_bytes / (t["gram"] * 1e-3) / HBM_PEAK,
            "eig_jacobi_ms": t["jacobi"], "eig_jacobi_unconverged": unconv, "eig_rocsolver_ms": t["rocsolver"],
            "map_ms": t["map"], "project_ms": t["project"],
            "project_hbm_fraction": proj_bytes / (t["project"] * 1e-3) / HBM_PEAK,
            "form_jacobi_ms": form["jacobi"], "form_rocsolver_ms": form["rocsolver"],
            "rp_factor_ms": med([v[0] for v in rp_f]), "rp_factor_sweeps_mean": float(st_f[1][:, 1].mean()),
            "rp_factor_ok": int((st_f[2] == _lib.PQ_RP_OK).sum().item()),
            "hrp_factor_cov_ms": med([v[0] for v in hf]), "hrp_factor_kernel_ms": med([v[1] for v in hf]),
            "hrp_factor_ok": hf[-1][2], **base}), flush=True)


if __name__ == "__main__":
    main()
