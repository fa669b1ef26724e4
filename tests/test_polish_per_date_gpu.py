"""The per-date polish kernels k_polish_w (polish_w.hip) and k_polish (polish.hip) on manufactured
optima (tests/manufactured.py), called directly: ws.x, ws.z, ws.y are filled from
manufactured.start_state (x* with x_F moved by 1e-7, the rows and the box classified exactly as
constructed by start_box / start_row), ws.status = PQ_SOLVED, lr.mu are the device's own window means
and the optima are built from those.  No ADMM runs, so the free-set size k, the mode, the start
distance and the starting classification are inputs of the test, and only the end state is compared
-- with x*, lambda, z themselves.  Batches: manufactured.PER_DATE, n = 300 (ld 320) on consecutive
daily windows, every date with a ridge of 4 x mean diag P.

  compact (k <= ldk = 256)   cA k = 2, 63, 64, 65, 127, 128, 129, 192, 193, 256 at T = 120 (form_pff_small<1>, <2>,
        form_pff and their tile edges); cT20 / 32 / 33 / 65: k = 100 at those T (form_pff_small's 32-row chunks,
        its double buffer, T no multiple of 16); cB box [0, 0.05] with weights at ub (nzb: P x_B through the
        window, full_px); cW uncentred, box [-1, 1]; cK0 every weight at a bound; cR16 / cR32 40 disjoint groups
        and the budget, ma = 17 and 33 at k = 120 (the Schur complement beyond 9 rows); cN no general row, k = 1,
        64, 130, 256; cBig n = 1027 (a second, ragged 1024-column chunk of lr_pass1 / lr_pass2), T = 60, k = 64, 200.
        Under a budget row and a shared box a single free variable is at a bound, never inside the box (it
        carries 1 minus a multiple of the box width), so k = 1 is the box-only batch's.
  Woodbury (k > ldk >= 64 ceil(T / 64))   wA, wW (uncentred, fixed weights at +-1: nzb) T = 120, ldk = 128,
        n - k = 0, 1, 7, 8, 9, 128, 129 fixed columns: with the band of engine._band_setup the gather and the
        DC = 8 chunks of form_cwood_band's downdate, 129 falls back to form_cwood; the same dates with band =
        NULL; wT64 / wT60 (ldk = 64: one capacitance tile, full and padded), wT65 (ldk = 128); wN ma = 0,
        wC8 ma = 9; fixed weights at 0 in the A batches (the px_ready shortcut).
  overflow   oA: T = 120, ldk = 64, k = 65, 129, 200 next to 30 and 64: ROUNDS = -1 and the state bitwise as it
        was; the relaunch as engine._LowRankSolve.polish_w does it (idx list in either order, one K / Dt slot
        per listed problem, ldk = ld); final_try = 1 on the first launch.
  dense   pq_polish_batched and pq_polish_lr_batched on P64 = the float64 rounding of the window's P, ridge as
        p_diag, optima of exactly that matrix: dA n = 301, k = 0, 64, 65, 200, 301; dN no general row, k = 1, 65;
        dA1024 n = 1024, k = 64, 200, 1024; dC8 ma = 9; dU no box.
  multi-round   fA (compact), fW (Woodbury): one variable per date starts wrongly classified
        (manufactured.flip_start); PQ_OUT_ROUNDS is the count of tests/engine_model.py's polish.
  engine leg   eC, eW: engine.solve_lowrank(grouped_polish=False) with eps 1e-7, Workspace(kcap=64), T = 60.

Every case first asserts the mode it claims from PQ_OUT_NFREE, ldk, T and the band argument (_mode).

Bars (the standing ones of tests/test_polish_buckets_gpu.py).  (a) exact: status SOLVED, NFREE = k_d,
{i: lb < x_i < ub} = F, z_box zero exactly there, ROUNDS = 1 from a correctly classified start.
(b) parity: weights 1e-5 L-inf, objective 1e-6 relative, violation 1e-7, and the certificate bars of
workloads.window_certificate (violation 1e-9; stationarity, complementarity, dual sign 1e-8; the dense
and the row-less batches through tests/kkt.py on the host, same bars).  (c) model distance, per date:

    |x - x*|inf / |x*|inf  <=  10 d_model + 1e-14,    the same for (lambda, z_box) relative to s

d_model the same distance of the float64 yardstick of the batch's mode (reduced_kkt_f64: compact and,
on P_FF of the dense matrix, dense; reduced_kkt_woodbury_f64: Woodbury) from the same start with the
same refinement count, 10 d_model <= 1e-9 asserted; with refine_iters = 1 and = refine_retry.
tests/test_manufactured.py holds the CPU side (uniqueness, start classification, d_model, flip rounds).

Measured on an MI355X, refine_iters = 1 and = refine_retry alike (254 date-runs under bar (c)): every
date SOLVED in one round in the mode it claims; one refinement step in model and kernel (the stop rule
ends the Woodbury mode's second).  Worst |x - x*|inf 8.9e-16 (compact), 9.0e-16 (Woodbury), 3.0e-17
(dense), 1.9e-17 (overflow / relaunch); objective <= 1.1e-15 relative, violation <= 2.2e-15, certificate
stationarity <= 6.5e-16.  Flipped starts: kernel rounds = model rounds on all 24 date-runs (2, and 3 on
the k = 256 and k = 292 dates), worst |x - x*|inf 3.3e-11, stationarity 1.6e-10.  Engine leg (41 .. 46 ADMM
iterations, capacitance "band"): eC compact x 3, eW form_cwood (n - k = 200) and band (n - k = 100), one round.
Bar (c), worst d_kernel / d_model per path (d_kernel / d_model of that date); CPU d_model of the batches,
worst: compact 5.3e-15, Woodbury 5.3e-15, dense 4.3e-14 (tests/test_manufactured.py):
                              x                             multipliers
  compact form_pff_small<1>   1.35  (7.5e-16 / 5.5e-16)     1.83  (4.5e-16 / 2.5e-16)
  compact form_pff_small<2>   1.24  (1.7e-15 / 1.3e-15)     1.11  (5.3e-16 / 4.8e-16)
  compact form_pff            1.04  (3.7e-16 / 3.5e-16)     1.26  (2.5e-16 / 1.9e-16)
  woodbury form_cwood         1.21  (8.3e-16 / 6.8e-16)     2.09  (2.6e-16 / 1.3e-16)
  woodbury band               1.20  (4.3e-15 / 3.6e-15)     2.09  (2.6e-16 / 1.3e-16)
  dense                       1.00  (1.6e-17 / 1.6e-17)     1.72  (3.4e-16 / 2.0e-16)
No kernel missed a bar and none was changed.  What bar (c) sees, measured: a build whose
form_cwood_band leaves the last fixed column out of the downdate applies a slightly wrong A^-1; the
refinement's exact residuals still pull it towards x*, so bars (a) and (b) pass, but the band dates with
n - k >= 1 end at d_kernel 4.9e-11 (x) and 7.8e-11 (multipliers) against d_model 3.8e-15 and 2.1e-16
(refine_retry: 3.0e-12 and 2.5e-13) and fail bar (c) in wA and wW; nothing else in the suite reads that
path below 1e-5.
"""
import ctypes
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.workloads import window_certificate
from tests import manufactured as mf
from tests.kkt import kkt_residuals

pytestmark = pytest.mark.gpu
F64 = torch.float64
LD = np.longdouble
REFINES = ("default", "retry")
RATIOS = {}           # path -> what -> [worst d_kernel / d_model, d_kernel, d_model] (bar c)


def _settings(refine, **kw):
    st = engine.Settings(**kw)
    return dataclasses.replace(st, refine_iters=st.refine_retry) if refine == "retry" else st


@dataclasses.dataclass
class Prob:
    b: mf.Batch
    pan: engine.Panel
    qb: engine.QPBatch
    lr: engine.LowRank


@functools.lru_cache(maxsize=None)
def _problem(device, name) -> Prob:
    """The batch on the device, its optima manufactured with the device's own window means."""
    c = mf.PER_DATE[name]
    bw = mf.family_windows(c["fam"], c["n"], c["t"], c["sizes"])
    n, D = bw.n, bw.D
    pan = engine.Panel(bw.R, device=device)
    if n % 2:   # the window form reads an even panel stride
        wide = torch.zeros((pan.R.shape[0], n + 1), dtype=F64, device=device)
        wide[:, :n] = pan.R
        pan.R = wide[:, :n]
    r_d, t_d = pan.rows_to_device(bw.rows, bw.tlen)
    mu = pan.window_means(r_d, t_d) if bw.centred else None
    b = mf.per_date(name, mu=None if mu is None else mu[:, :n].cpu().numpy().copy())
    mg, box, dense = b.C.shape[0], bool(np.isfinite(b.lb).all()), b.mode == "dense"
    G = b.C[1:] if mg > 1 else None
    qb = engine.QPBatch.from_dense(None, None, A=b.C[:1] if mg else None, b=b.ug[:1] if mg else None, G=G,
                                   h=None if G is None else b.ug[1:], lb=b.lb if box else None,
                                   ub=b.ub if box else None, device=device, n=n)
    assert qb.mg == mg and qb.has_box == box and qb.shared
    qb.batch = D
    qb.p_scale = None if dense else torch.full((D,), b.p_scale, dtype=F64, device=device)
    qb.p_diag = torch.tensor([o.p_diag for o in b.opt], dtype=F64, device=device)
    q = np.zeros((D, qb.ld))
    q[:, :n] = np.stack([o.q for o in b.opt])
    qb.q = torch.from_numpy(q).to(device)
    if dense:
        P = np.zeros((D, qb.ld, qb.ld))
        P[:, :n, :n] = np.stack(b.P)
        qb.P = torch.from_numpy(P).to(device)
    w = 1.0 / (t_d.to(F64) - 1.0) if bw.centred else None
    if dense:   # p_scale = 1: the window's whole scale is w_scale
        w = b.p_scale * w
    lr = engine.LowRank(pan, r_d, t_d, mu=mu, w_scale=w)
    return Prob(b, pan, qb, lr)


def _fill(p: Prob, ws, starts):
    """ws.x / z / y from the start points (rows [general; box] -> the state's [mg_pad | ld] layout), SOLVED."""
    b, qb = p.b, p.qb
    n, mg, mp = b.n, b.C.shape[0], ws.mg_pad
    x, z, y = np.zeros((b.D, qb.ld)), np.zeros((b.D, ws.m_ld)), np.zeros((b.D, ws.m_ld))
    for d, s in enumerate(starts):
        x[d, :n] = s[0]
        for dst, src in ((z, s[1]), (y, s[2])):
            dst[d, :mg] = src[:mg]
            dst[d, mp:mp + n] = src[mg:]
    for t, v in ((ws.x, x), (ws.z, z), (ws.y, y)):
        t.copy_(torch.from_numpy(v))
    ws.status.fill_(_lib.PQ_SOLVED)
    ws.out.zero_()
    torch.cuda.synchronize()


def _read(p: Prob, ws):
    torch.cuda.synchronize()
    n, mg, mp = p.b.n, p.b.C.shape[0], ws.mg_pad
    raw = {k: getattr(ws, k).cpu().numpy().copy() for k in ("x", "z", "y", "status", "out")}
    return dict(raw=raw, x=raw["x"][:, :n], y=raw["y"][:, :mg], zb=raw["y"][:, mp:mp + n], zr=raw["z"][:, :mg],
                status=raw["status"], out=raw["out"])


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch_w(p: Prob, ws, st, ldk, final_try=0, idx=None, band=None, K=None, Dt=None):
    lib = _lib.load()
    L, P, S, s = p.lr.c_struct(), p.qb.c_struct(), ws.c_struct(K, Dt), st.to_c()
    bk = band if band is not None else (None, 0, 0)
    _lib.check(lib.pq_polish_w_batched(ctypes.byref(L), ctypes.byref(P), ctypes.byref(S),
                                       None if idx is None else idx.data_ptr(), 0 if idx is None else int(idx.numel()),
                                       ctypes.byref(s), ldk, final_try, *bk, _strm()), "pq_polish_w_batched")
    torch.cuda.synchronize()


def _mode(k, ldk, T, n, band):
    """The mode k_polish_w takes for a free set of k: its own conditions, restated."""
    if k <= min(ldk, 1024):
        return "compact"
    if 64 * math.ceil(T / 64) <= ldk:
        return "woodbury band" if band and n - k <= 128 else "woodbury form_cwood"
    return "overflow"


def _path(b, k, ldk, band):
    m = "dense" if b.mode == "dense" else _mode(k, ldk, int(b.tlen[0]), b.n, band)
    if m == "compact":
        m += " form_pff_small<1>" if k <= 64 else " form_pff_small<2>" if k <= 128 else " form_pff"
    return m


def _bar_a(tag, b, r, dates, rounds=1):
    for d in dates:
        o, x, zb = b.opt[d], r["x"][d], r["zb"][d]
        assert r["status"][d] == _lib.PQ_SOLVED, (tag, d, o.k, r["status"][d])
        assert r["out"][d, _lib.PQ_OUT_NFREE] == o.k, (tag, d, o.k, r["out"][d, _lib.PQ_OUT_NFREE])
        inside = np.flatnonzero((b.lb < x) & (x < b.ub))
        assert np.array_equal(inside, o.F), (tag, d, o.k, len(inside), np.setxor1d(inside, o.F))
        assert np.array_equal(np.flatnonzero(zb == 0.0), o.F), (tag, d, o.k)
        want = rounds if rounds is None or np.isscalar(rounds) else rounds[d]
        if want is not None:
            assert r["out"][d, _lib.PQ_OUT_ROUNDS] == want, (tag, d, o.k, r["out"][d, _lib.PQ_OUT_ROUNDS], want)


def _bar_b(tag, p: Prob, ws, r, dates):
    b, qb, lr = p.b, p.qb, p.lr
    n, mg = b.n, b.C.shape[0]
    eq = b.lg == b.ug
    box = bool(np.isfinite(b.lb).all())
    worst = dict(x=0.0, obj=0.0, viol=0.0)
    for d in dates:
        o, x = b.opt[d], r["x"][d]
        P = b.P64(d).astype(LD) if b.mode == "dense" else mf.window_P(b.X(d), None if b.mu is None else b.mu[d],
                                                                        b.psw(d), o.p_diag)
        obj_ref = float(0.5 * o.x @ (P @ o.x) + o.q.astype(LD) @ o.x)
        cx = b.C @ x
        viol = max(np.abs(cx - b.ug)[eq].max(initial=0.0), np.maximum(cx - b.ug, 0.0).max(initial=0.0),
                   np.maximum(b.lb - x, 0.0).max(), np.maximum(x - b.ub, 0.0).max())
        e = dict(x=float(np.abs(x - o.x).max()), obj=abs(r["out"][d, _lib.PQ_OUT_OBJ] - obj_ref) / abs(obj_ref),
                 viol=float(viol))
        assert e["x"] <= 1e-5 and e["obj"] <= 1e-6 and e["viol"] <= 1e-7, (tag, d, o.k, e)
        worst = {k: max(worst[k], e[k]) for k in worst}
    if b.mode != "dense" and mg and len(dates) == b.D:
        res = engine._batch_result(qb, ws)
        c = window_certificate(p.pan.R, lr.rows, lr.tlen, lr.mu, qb.p_scale * (lr.w_scale if lr.w_scale is not None else 1.0),
                               qb.q[:, :n], res, lb=qb.lb[0, :n], ub=qb.ub[0, :n], C=qb.Cg[0, :mg, :n],
                               lg=qb.lg[0, :mg], ug=qb.ug[0, :mg], p_diag=qb.p_diag)
    else:   # tests/kkt.py on the host, from the float64 matrix
        c = dict(max_violation=0.0, max_rel_stationarity=0.0, max_rel_complementarity=0.0, max_dual_sign=0.0)
        for d in dates:
            k = kkt_residuals(b.P64(d), b.opt[d].q, r["x"][d], A=b.C[eq] if eq.any() else None,
                              b=b.ug[eq] if eq.any() else None, G=b.C[~eq] if (~eq).any() else None,
                              h=b.ug[~eq] if (~eq).any() else None, lb=b.lb if box else None, ub=b.ub if box else None,
                              y=np.concatenate([r["y"][d][eq], r["y"][d][~eq]]), z_box=r["zb"][d])
            for f, g in (("max_violation", "prim"), ("max_rel_stationarity", "stat"), ("max_rel_complementarity", "comp"),
                         ("max_dual_sign", "dual")):
                c[f] = max(c[f], k[g])
    print(f"[per-date] {tag}: worst |x - x*| {worst['x']:.1e}  obj {worst['obj']:.1e}  violation {worst['viol']:.1e}  "
          f"certificate viol {c['max_violation']:.1e} stat {c['max_rel_stationarity']:.1e} "
          f"comp {c['max_rel_complementarity']:.1e}")
    assert c["max_violation"] <= 1e-9, (tag, c)
    assert c["max_rel_stationarity"] <= 1e-8 and c["max_rel_complementarity"] <= 1e-8 and c["max_dual_sign"] <= 1e-8, (tag, c)


def _bar_c(tag, b, r, starts, st, dates, ldk, band=False):
    mg = b.C.shape[0]
    missed = []
    for d in dates:
        o = b.opt[d]
        (xm, lm, zm, steps), _ = mf.per_date_model(b, d, starts[d][0], starts[d][2][:mg], st.delta, st.refine_iters)
        xs = np.abs(o.x).max()
        dist = lambda x, lam, zb: (float(np.abs(x - o.x).max() / xs),
                                   float(max(np.abs(lam - o.lam).max(initial=0.0), np.abs(zb - o.z).max()) / o.s))
        dk, dm = dist(r["x"][d], r["y"][d], r["zb"][d]), dist(xm, lm, zm)
        path = _path(b, o.k, ldk, band)
        print(f"[per-date] bar (c) {tag} date {d:2d} k {o.k:4d} ma {int(o.act.sum()):2d} {path:26s} model steps {steps}  "
              f"x {dk[0]:.1e} / {dm[0]:.1e}  multipliers {dk[1]:.1e} / {dm[1]:.1e}")
        for what, k_, m_ in zip(("x", "multipliers"), dk, dm):
            s = RATIOS.setdefault((path, what), [0.0, 0.0, 0.0])
            ratio = k_ / max(m_, 1e-300)
            if ratio > s[0]:
                s[:] = [ratio, k_, m_]
            assert 10.0 * m_ <= 1e-9, (tag, d, o.k, what, m_)
            if not k_ <= 10.0 * m_ + 1e-14:
                missed.append((d, o.k, path, what, k_, m_))
    for (path, what), s in sorted(RATIOS.items()):
        print(f"[per-date] bar (c) so far {path:28s} {what:11s} worst d_kernel / d_model {s[0]:8.2f} ({s[1]:.1e} / {s[2]:.1e})")
    assert not missed, (tag, missed)


def _claim_modes(tag, b, r, ldk, band, want):
    """Every date ran in the mode the case claims (from PQ_OUT_NFREE, ldk, T, band)."""
    T = int(b.tlen[0])
    got = [_mode(int(r["out"][d, _lib.PQ_OUT_NFREE]), ldk, T, b.n, band) for d in range(b.D)]
    assert all(g in want for g in got), (tag, got, want)
    return got


# ----------------------------------------------------------------------------------------
# pq_polish_w_batched, compact mode
# ----------------------------------------------------------------------------------------

COMPACT = ("cA", "cT20", "cT32", "cT33", "cT65", "cB", "cW", "cR16", "cR32", "cN", "cBig")


@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("name", COMPACT)
def test_compact_mode(device, name, refine):
    p = _problem(device, name)
    b, st = p.b, _settings(refine)
    ws = engine.Workspace(p.qb, dense=False, kcap=b.ldk)
    assert ws.ldk == b.ldk == 256
    starts = [mf.start_state(b, d) for d in range(b.D)]
    _fill(p, ws, starts)
    _launch_w(p, ws, st, ws.ldk)
    r = _read(p, ws)
    tag, dates = f"{name} {refine}", range(b.D)
    assert set(_claim_modes(tag, b, r, ws.ldk, False, {"compact"})) == {"compact"}
    _bar_a(tag, b, r, dates)
    _bar_b(tag, p, ws, r, dates)
    _bar_c(tag, b, r, starts, st, dates, ws.ldk)


def _sum_tol(b, o, lam):
    """Float64 evaluation of g = P x + q + C' lam, an n-term sum of terms of these sizes: n u of their scale."""
    return b.n * np.finfo(np.float64).eps * (o.s + float(np.abs(o.q).max()) + abs(float(lam)))


def test_every_weight_at_a_bound(device):
    """k = 0: the budget row has no free support, so nothing is solved -- x is the bounds exactly, lambda
    stays at the start point's and z_box = -g of that lambda."""
    p = _problem(device, "cK0")
    b, st = p.b, _settings("default")
    ws = engine.Workspace(p.qb, dense=False, kcap=b.ldk)
    starts = [mf.start_state(b, d) for d in range(b.D)]
    _fill(p, ws, starts)
    _launch_w(p, ws, st, ws.ldk)
    r = _read(p, ws)
    assert _claim_modes("cK0", b, r, ws.ldk, False, {"compact"})
    for d, o in enumerate(b.opt):
        assert o.k == 0 and r["status"][d] == _lib.PQ_SOLVED and r["out"][d, _lib.PQ_OUT_NFREE] == 0
        assert r["out"][d, _lib.PQ_OUT_ROUNDS] == 1
        assert np.array_equal(r["x"][d], np.where(o.side == 1, b.lb, b.ub))
        lam0 = starts[d][2][:1]
        assert np.array_equal(r["y"][d], lam0), (d, r["y"][d], lam0)
        P = mf.window_P(b.X(d), b.mu[d], b.psw(d), o.p_diag)
        g = P @ r["x"][d].astype(LD) + o.q.astype(LD) + b.C[0].astype(LD) * LD(lam0[0])
        assert np.abs(r["zb"][d] + g).max() <= _sum_tol(b, o, lam0[0]), (d, float(np.abs(r["zb"][d] + g).max() / o.s))
        assert np.all(r["zb"][d] != 0.0)


# ----------------------------------------------------------------------------------------
# pq_polish_w_batched, Woodbury mode
# ----------------------------------------------------------------------------------------

WOODBURY = [(n, False) for n in ("wA", "wW", "wT64", "wT60", "wT65", "wN", "wC8")] + \
           [(n, True) for n in ("wA", "wW", "wT64", "wT60", "wT65")]


@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("name,band", WOODBURY)
def test_woodbury_mode(device, name, band, refine):
    p = _problem(device, name)
    b, st = p.b, _settings(refine)
    T = int(b.tlen[0])
    ws = engine.Workspace(p.qb, dense=False, kcap=b.ldk)
    assert ws.ldk == b.ldk and 64 * math.ceil(T / 64) <= ws.ldk < min(o.k for o in b.opt)
    bk = None
    if band:
        bd = engine._band_setup(p.qb, p.lr, _strm())
        assert bd is not None
        bk = bd["cap"][:3]
    starts = [mf.start_state(b, d) for d in range(b.D)]
    _fill(p, ws, starts)
    _launch_w(p, ws, st, ws.ldk, band=bk)
    r = _read(p, ws)
    tag, dates = f"{name} {'band' if band else 'form_cwood'} {refine}", range(b.D)
    got = _claim_modes(tag, b, r, ws.ldk, band, {"woodbury band", "woodbury form_cwood"})
    if band:   # the gather with 0 .. 128 fixed columns; more fall back to form_cwood
        assert got == ["woodbury band" if b.n - o.k <= 128 else "woodbury form_cwood" for o in b.opt], got
        assert "woodbury band" in got
        if name in ("wA", "wW"):
            assert [b.n - o.k for o in b.opt] == [0, 1, 7, 8, 9, 128, 129] and got[-1] == "woodbury form_cwood"
    else:
        assert set(got) == {"woodbury form_cwood"}
    _bar_a(tag, b, r, dates)
    _bar_b(tag, p, ws, r, dates)
    _bar_c(tag, b, r, starts, st, dates, ws.ldk, band)


# ----------------------------------------------------------------------------------------
# pq_polish_w_batched, overflow and relaunch
# ----------------------------------------------------------------------------------------


def _overflow_first_launch(p, st, final_try):
    b = p.b
    ws = engine.Workspace(p.qb, dense=False, kcap=64)
    assert ws.ldk == 64 and int(b.tlen[0]) == 120
    starts = [mf.start_state(b, d) for d in range(b.D)]
    _fill(p, ws, starts)
    r0 = _read(p, ws)
    _launch_w(p, ws, st, 64, final_try=final_try)
    r = _read(p, ws)
    modes = _claim_modes("oA", b, r, 64, False, {"compact", "overflow"})
    assert modes == ["compact" if o.k <= 64 else "overflow" for o in b.opt] and modes.count("overflow") == 3
    return ws, starts, r0, r, modes


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("refine", REFINES)
def test_overflow_leaves_the_state_for_the_relaunch(device, refine, order):
    p = _problem(device, "oA")
    b, st = p.b, _settings(refine)
    ws, starts, r0, r, modes = _overflow_first_launch(p, st, 0)
    over = [d for d in range(b.D) if modes[d] == "overflow"]
    fit = [d for d in range(b.D) if modes[d] == "compact"]
    for d in over:
        assert r["out"][d, _lib.PQ_OUT_ROUNDS] == -1 and r["out"][d, _lib.PQ_OUT_NFREE] == b.opt[d].k
        for f in ("x", "z", "y", "status"):
            assert np.array_equal(r["raw"][f][d], r0["raw"][f][d]), (d, f)
    tag = f"oA first launch {refine}"
    _bar_a(tag, b, r, fit)
    _bar_b(tag, p, ws, r, fit)
    _bar_c(tag, b, r, starts, st, fit, 64)
    # the relaunch of engine._LowRankSolve.polish_w: one K / Dt slot per listed problem, ldk = min(ld, 1024)
    kmax = min(p.qb.ld, 1024)
    lst = over if order == "ascending" else over[::-1]
    idx = torch.tensor(lst, dtype=torch.int32, device=p.qb.device)
    K2 = torch.empty((len(lst), kmax, kmax), dtype=F64, device=p.qb.device)
    D2 = torch.empty((len(lst), kmax // 64, 64, 64), dtype=F64, device=p.qb.device)
    _launch_w(p, ws, st, kmax, final_try=1, idx=idx, K=K2, Dt=D2)
    r2 = _read(p, ws)
    for d in fit:   # not listed: bitwise untouched
        for f in ("x", "z", "y", "status", "out"):
            assert np.array_equal(r2["raw"][f][d], r["raw"][f][d]), (d, f)
    tag = f"oA relaunch {order} {refine}"
    assert [_mode(b.opt[d].k, kmax, 120, b.n, False) for d in over] == ["compact"] * len(over)
    _bar_a(tag, b, r2, range(b.D))
    _bar_b(tag, p, ws, r2, range(b.D))
    _bar_c(tag, b, r2, starts, st, over, kmax)


def test_overflow_on_the_final_try_scores_the_start_point(device):
    p = _problem(device, "oA")
    b, st = p.b, _settings("default")
    ws, starts, r0, r, modes = _overflow_first_launch(p, st, 1)
    for d in range(b.D):
        if modes[d] == "overflow":
            assert r["status"][d] == _lib.PQ_SOLVED_INACCURATE and r["out"][d, _lib.PQ_OUT_NFREE] == b.opt[d].k
            assert np.array_equal(r["x"][d], r0["x"][d]) and np.array_equal(r["zb"][d], r0["zb"][d])
            assert np.array_equal(r["y"][d], r0["y"][d])
        else:
            assert r["status"][d] == _lib.PQ_SOLVED
    _bar_a("oA final_try", b, r, [d for d in range(b.D) if modes[d] == "compact"])


# ----------------------------------------------------------------------------------------
# the dense kernel: pq_polish_batched, pq_polish_lr_batched
# ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("entry", ["pq_polish_batched", "pq_polish_lr_batched"])
@pytest.mark.parametrize("name", ["dA", "dN", "dA1024", "dC8", "dU"])
def test_dense_kernel(device, name, entry, refine):
    p = _problem(device, name)
    b, st = p.b, _settings(refine)
    assert p.qb.P is not None and p.qb.p_scale is None and p.qb.has_box == (name != "dU")
    ws = engine.Workspace(p.qb)
    starts = [mf.start_state(b, d) for d in range(b.D)]
    _fill(p, ws, starts)
    lib = _lib.load()
    P, S, s, L = p.qb.c_struct(), ws.c_struct(), st.to_c(), p.lr.c_struct()
    if entry == "pq_polish_batched":
        _lib.check(lib.pq_polish_batched(ctypes.byref(P), ctypes.byref(S), None, 0, ctypes.byref(s), _strm()), entry)
    else:
        _lib.check(lib.pq_polish_lr_batched(ctypes.byref(L), ctypes.byref(P), ctypes.byref(S), None, 0, ctypes.byref(s),
                                            _strm()), entry)
    r = _read(p, ws)
    tag = f"{name} {entry} {refine}"
    solved = [d for d in range(b.D) if b.opt[d].k > 0]
    _bar_a(tag, b, r, solved)
    _bar_b(tag, p, ws, r, solved)
    _bar_c(tag, b, r, starts, st, solved, p.qb.ld)
    for d in set(range(b.D)) - set(solved):   # k = 0: as in test_every_weight_at_a_bound
        o = b.opt[d]
        assert r["status"][d] == _lib.PQ_SOLVED and r["out"][d, _lib.PQ_OUT_NFREE] == 0
        assert np.array_equal(r["x"][d], np.where(o.side == 1, b.lb, b.ub))
        assert np.array_equal(r["y"][d], starts[d][2][:1])
        g = b.P64(d).astype(LD) @ r["x"][d].astype(LD) + o.q.astype(LD) + b.C[0].astype(LD) * LD(r["y"][d][0])
        assert np.abs(r["zb"][d] + g).max() <= _sum_tol(b, o, r["y"][d][0])


# ----------------------------------------------------------------------------------------
# multi-round dates
# ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("name", ["fA", "fW"])
def test_wrongly_classified_start_takes_the_models_rounds(device, name, refine):
    p = _problem(device, name)
    b, st = p.b, _settings(refine)
    steps = max(st.refine_iters, 2) if b.mode == "woodbury" else st.refine_iters
    flips = [mf.flip_start(b, d, delta=st.delta, dual_tol=st.dual_tol, rounds=st.polish_rounds, refine=steps)
             for d in range(b.D)]
    assert all(f is not None for f in flips)
    ws = engine.Workspace(p.qb, dense=False, kcap=b.ldk)
    _fill(p, ws, flips)
    _launch_w(p, ws, st, ws.ldk)
    r = _read(p, ws)
    tag = f"{name} {refine}"
    want = {"woodbury form_cwood"} if b.mode == "woodbury" else {"compact"}
    assert set(_claim_modes(tag, b, r, ws.ldk, False, want)) == want
    print(f"[per-date] {tag}: (k, flipped, kind, model rounds, kernel rounds) "
          f"{[(o.k,) + f[3:] + (int(r['out'][d, _lib.PQ_OUT_ROUNDS]),) for d, (o, f) in enumerate(zip(b.opt, flips))]}")
    _bar_a(tag, b, r, range(b.D), rounds=[f[5] for f in flips])
    _bar_b(tag, p, ws, r, range(b.D))


# ----------------------------------------------------------------------------------------
# one engine leg: the real ADMM reaches the modes pinned above
# ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,mode", [("eC", "compact"), ("eW", "woodbury band")])
def test_engine_reaches_the_mode(device, name, mode):
    p = _problem(device, name)
    b = p.b
    st = engine.Settings(eps_abs=1e-7, eps_rel=1e-7)
    ws = engine.Workspace(p.qb, dense=False, kcap=64)
    assert ws.ldk == 64 and int(b.tlen[0]) == 60
    res = engine.solve_lowrank(p.qb, p.lr, st, ws=ws, grouped_polish=False)
    r = _read(p, ws)
    band = res.capacitance == "band"
    got = _claim_modes(name, b, r, 64, band, {mode, "woodbury form_cwood"} if mode != "compact" else {mode})
    print(f"[per-date] engine leg {name}: capacitance {res.capacitance}, modes {got}, ADMM iterations "
          f"{res.iters.cpu().numpy().tolist()}, rounds {r['out'][:, _lib.PQ_OUT_ROUNDS].tolist()}")
    _bar_a(name, b, r, range(b.D), rounds=None)
    assert np.all((1 <= r["out"][:, _lib.PQ_OUT_ROUNDS]) & (r["out"][:, _lib.PQ_OUT_ROUNDS] <= st.polish_rounds))
    _bar_b(name, p, ws, r, range(b.D))
