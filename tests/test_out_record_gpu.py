"""The engine's self-reported certificate out[PQ_OUT_OBJ | PRIM | DUAL | GAP | NFREE | ROUNDS]
against an independent extended-precision model of the same definitions
(tests/residual_model.py), on every kernel that writes it: k_polish (polish.hip, dense and
with P x from the window), k_polish_w (polish_w.hip: compact, relaunch and Woodbury modes, and
the ADMM-point scoring of a rejected polish), k_pg_post (polish_g.hip) behind its four round
solvers (register tile, LDS, k_pg_big, wide rounds), and the host residuals of the device IPM
route (qp_problems._solve_batch_ipm).  The bar is the model's derived N u S -- not a measured
one -- so a scoring block that pairs the final x with a stale P x or g, a wrong sign or bound in
the gap, or a z_box written for another point fails by orders of magnitude.  Each test prints
the largest observed |engine - model| / (u S) per field (pytest -s): observations next to the
bar N, recorded in profiles/ and DESIGN.md."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle.qp_ipm import OracleSolution
from oracle.ref_pipeline import cov_pearson
from porqua_amd import _lib, engine
from porqua_amd.qp_problems import QuadraticProgram, batch_result_to_solutions, solve_batch
from porqua_amd.synthetic import factor_panel
from tests import residual_model as rm
from tests import window_cases as wc
from tests.kkt import kkt_residuals
from tests.test_polish_grouped_gpu import _problem as grouped_problem
from tests.test_polish_wide_gpu import _problem as wide_problem
from tests.test_window_polish_gpu import _mv_batch

pytestmark = pytest.mark.gpu
F64 = torch.float64
OUT = {"obj": _lib.PQ_OUT_OBJ, "prim": _lib.PQ_OUT_PRIM, "dual": _lib.PQ_OUT_DUAL, "gap": _lib.PQ_OUT_GAP}


# ----------------------------------------------------------------------------------------
# the shared helper: host copy of a batch, the model per problem, the assertions
# ----------------------------------------------------------------------------------------


class Host:
    """Host copy of a QPBatch (and its LowRank window, when P is in window form)."""

    def __init__(self, qb, lr=None):
        n, mg, B = qb.n, qb.mg, qb.batch
        self.n, self.mg, self.B, self.box = n, mg, B, qb.lb is not None
        np_ = lambda t: t.detach().cpu().numpy().copy()
        self.q = np_(qb.q[:, :n])
        self.C, self.lg, self.ug = np_(qb.Cg[:, :mg, :n]), np_(qb.lg[:, :mg]), np_(qb.ug[:, :mg])
        if self.box:
            self.lb, self.ub = np_(qb.lb[:, :n]), np_(qb.ub[:, :n])
        self.ps = np_(qb.p_scale) if qb.p_scale is not None else np.ones(B)
        self.pd = np_(qb.p_diag) if qb.p_diag is not None else np.zeros(B)
        self.window = lr is not None
        if self.window:
            self.R = np_(lr.panel.R)
            self.rows, self.tlen = np_(lr.rows), np_(lr.tlen)
            self.mu = np_(lr.mu[:, :n]) if lr.mu is not None else None
            ws_ = lr.w_scale
            self.wsc = np.ones(B) if ws_ is None else (np_(ws_) if isinstance(ws_, torch.Tensor) else np.full(B, ws_))
            self.dg = np_(lr.dg[:, :n])
        else:
            self.P = np_(qb.P[:, :n, :n])

    def sc(self, i):
        """The kernels' problem scale in their own float64 arithmetic and from their own inputs:
        max(||q||inf, max_i |P_eff,ii|), diag P from P itself or from the window's sums of squares (lr.dg)."""
        d = (self.ps[i] * self.wsc[i]) * self.dg[i] if self.window else self.ps[i] * np.diag(self.P[i])
        return max(float(np.abs(self.q[i]).max()), float(np.abs(d + self.pd[i]).max()), 1e-300)

    def rows_of(self, i):
        j = 0 if self.C.shape[0] == 1 else i
        if not self.mg:
            return None, None, None
        return self.C[j], self.lg[j], self.ug[j]

    def box_of(self, i):
        if not self.box:
            return None, None
        j = 0 if self.lb.shape[0] == 1 else i
        return self.lb[j], self.ub[j]

    def X(self, i):
        return self.R[self.rows[i, :self.tlen[i]]]

    def record(self, i, x, y, zb) -> rm.Record:
        C, lg, ug = self.rows_of(i)
        lb, ub = self.box_of(i)
        kw = dict(y=y if self.mg else None, z_box=zb if self.box else None, C=C, lg=lg, ug=ug, lb=lb, ub=ub,
                  p_scale=self.ps[i], p_diag=self.pd[i])
        if self.window:
            return rm.window_record(self.X(i), None if self.mu is None else self.mu[i], self.q[i], x,
                                    w_scale=self.wsc[i], **kw)
        return rm.dense_record(self.P[i], self.q[i], x, **kw)

    def P_eff(self, i):
        """P_eff as a float64 matrix (for the KKT certificate, tests/kkt.py)."""
        if not self.window:
            return self.ps[i] * self.P[i] + self.pd[i] * np.eye(self.n)
        Xc = self.X(i) if self.mu is None else self.X(i) - self.mu[i][None, :]
        return self.ps[i] * self.wsc[i] * (Xc.T @ Xc) + self.pd[i] * np.eye(self.n)


def _certificate(P, q, x, y, zb, C, lg, ug, lb, ub):
    """tests/kkt.py on the engine's row storage: equality rows -> A x = b, a finite ug -> a row of
    G x <= h with its y+, a finite lg -> a row of -C x <= -lg with its y-.  An infinite box side is
    replaced by a bound at distance 1, so a multiplier on it counts in full as a complementarity error."""
    A = b = G = h = None
    ye, yg = np.zeros(0), np.zeros(0)
    if C is not None:
        eq = lg == ug
        A, b, ye = C[eq], ug[eq], y[eq]
        Gs, hs, ys = [], [], []
        for r in np.flatnonzero(~eq):
            if np.isfinite(ug[r]):
                Gs.append(C[r]); hs.append(ug[r]); ys.append(max(y[r], 0.0) if np.isfinite(lg[r]) else y[r])
            if np.isfinite(lg[r]):
                Gs.append(-C[r]); hs.append(-lg[r]); ys.append(max(-y[r], 0.0) if np.isfinite(ug[r]) else -y[r])
            assert np.isfinite(ug[r]) or np.isfinite(lg[r]) or y[r] == 0.0
        if Gs:
            G, h, yg = np.array(Gs), np.array(hs), np.array(ys)
        if not eq.any():
            A = b = None
    if lb is not None:
        lb = np.where(np.isfinite(lb), lb, x - 1.0)
        ub = np.where(np.isfinite(ub), ub, x + 1.0)
    return kkt_residuals(P, q, x, A=A, b=b, G=G, h=h, lb=lb, ub=ub, y=np.concatenate([ye, yg]),
                         z_box=zb if lb is not None else None)


STATS = {}   # route -> field -> largest |engine - model| / (u S) seen; route -> "N" -> the bar's N


def _note(route, rec, units):
    s = STATS.setdefault(route, {f: 0.0 for f in rm.FIELDS})
    for f in rm.FIELDS:
        s[f] = max(s[f], units[f])
    s["N"] = rec.N


def _report(prefix=""):
    for route in sorted(STATS):
        if route.startswith(prefix):
            s = STATS[route]
            print(f"[out-record] {route:34s} |engine - model| / (u S):  obj {s['obj']:7.2f}  prim {s['prim']:7.2f}  "
                  f"dual {s['dual']:7.2f}  gap {s['gap']:7.2f}   (bar N = {s['N']})")


def check_records(route, host, res, settings, routes=None, certify=True):
    """Pull the answers, run the model per problem, assert OBJ / PRIM / DUAL / GAP within N u S; for SOLVED
    problems also the statements that hold by construction of the scoring blocks and the KKT certificate.
    ``routes``: a label per problem (default: ``route`` for all).  Returns the host arrays."""
    torch.cuda.synchronize()
    x, y, zb = (t.detach().cpu().numpy().copy() for t in (res.x, res.y, res.z_box))
    status, out = res.status.cpu().numpy().copy(), res.out.cpu().numpy().copy()
    n = host.n
    for i in range(host.B):
        rec = host.record(i, x[i], y[i], zb[i])
        units = {f: rec.units(f, out[i, OUT[f]]) for f in rm.FIELDS}
        _note(routes[i] if routes is not None else route, rec, units)
        for f in rm.FIELDS:
            eng = out[i, OUT[f]]
            assert abs(rm.LD(eng) - rm.LD(rec.value(f))) <= rec.bar(f), \
                (route, i, f, eng, rec.value(f), f"{units[f]:.1f} u S against the bar N = {rec.N}", int(status[i]))
        if status[i] != _lib.PQ_SOLVED:
            continue
        C, lg, ug = host.rows_of(i)
        lb, ub = host.box_of(i)
        dtol = settings.dual_tol * host.sc(i)
        if host.box:
            inside = (lb < x[i]) & (x[i] < ub)
            assert np.all(zb[i][inside] == 0.0), (route, i, np.abs(zb[i][inside]).max())
            at_lo, at_up = (x[i] == lb) & (lb < ub), (x[i] == ub) & (ub > lb)
            assert np.all(zb[i][at_lo] <= dtol) and np.all(zb[i][at_up] >= -dtol), (route, i)
            nfree_lo, nfree_hi = int(inside.sum()), n - int((zb[i] != 0.0).sum())
        else:
            assert np.all(zb[i] == 0.0)
            nfree_lo = nfree_hi = n
        for r in range(host.mg):
            if lg[r] != ug[r] and np.isinf(lg[r]):
                assert y[i, r] >= -dtol, (route, i, r, y[i, r])
            if lg[r] != ug[r] and np.isinf(ug[r]):
                assert y[i, r] <= dtol, (route, i, r, y[i, r])
        assert nfree_lo <= out[i, _lib.PQ_OUT_NFREE] <= nfree_hi, (route, i, nfree_lo, out[i, _lib.PQ_OUT_NFREE], nfree_hi)
        assert 1 <= out[i, _lib.PQ_OUT_ROUNDS] <= settings.polish_rounds, (route, i, out[i, _lib.PQ_OUT_ROUNDS])
        if certify:
            c = _certificate(host.P_eff(i), host.q[i], x[i], y[i], zb[i], C, lg, ug, lb, ub)
            assert c["prim"] <= 1e-9, (route, i, c)
            assert c["stat"] <= 1e-8 and c["comp"] <= 1e-8 and c["dual"] <= 1e-8, (route, i, c)
    return x, y, zb, status, out


# ----------------------------------------------------------------------------------------
# a. dense k_polish through engine.solve
# ----------------------------------------------------------------------------------------


def _dense_batch(device, n, variant, B=3):
    T = n + 30                                     # P = cov of a T x n window: positive definite
    _, R, _, _ = factor_panel(T + 2 * B + 5, n)
    wins = [R[5 + 2 * i:5 + 2 * i + T] for i in range(B)]
    P = np.stack([cov_pearson(w) for w in wins])
    q = np.stack([-1.0 * w.mean(axis=0) for w in wins])
    third = np.arange(n) % 3
    kw = dict(A=np.ones((1, n)), b=np.ones(1), lb=np.zeros(n), ub=np.full(n, 0.2))
    caps = np.stack([(third == g).astype(float) for g in range(3)])
    tight = np.array([0.3, 0.35, 0.4])             # the thirds' caps leave 0.05 of slack in all: one binds
    if variant == "caps":                          # three one-sided rows
        kw.update(G=caps, h=tight)
    elif variant == "lowerside":                   # rows with a finite lg, set in the engine's storage below
        shunned = np.zeros(n)                      # the third of the assets with the lowest mean return: the
        shunned[np.argsort(q[0])[-(n // 3):]] = 1.0   # optimum holds little of them, so a floor on their sum binds
        kw.update(G=np.stack([caps[0], shunned, caps[2]]), h=tight)
    elif variant == "nobox":
        kw.update(lb=None, ub=None)
    elif variant == "infbox":                      # infinite sides: the isinf branches of the gap and prim sums
        kw.update(lb=np.where(third == 0, -np.inf, 0.0), ub=np.where(third == 1, np.inf, 0.2))
    elif variant == "perproblem":                  # shared = False: Cg_stride, g_stride, box_stride nonzero
        bud = np.array([1.0, 0.9, 1.1])[:B]
        kw.update(A=np.ones((B, 1, n)), b=bud[:, None],
                  G=np.stack([caps * (1.0 + 0.1 * i) for i in range(B)]),
                  h=np.stack([(1.0 + 0.1 * i) * bud[i] * np.roll(tight, i) for i in range(B)]),
                  lb=np.stack([np.full(n, -0.01 * i) for i in range(B)]),
                  ub=np.stack([np.full(n, 0.2 + 0.05 * i) for i in range(B)]))
    qb = engine.QPBatch.from_dense(2.0 * P if variant != "scaled" else P, q, device=device, **kw)
    if variant == "lowerside":   # first third capped from above, the shunned assets only from below (ug = +inf), last third two-sided
        qb.lg[0, 1:4] = torch.tensor([-np.inf, 0.38, 0.2], dtype=F64, device=device)
        qb.ug[0, 1:4] = torch.tensor([0.3, np.inf, 0.4], dtype=F64, device=device)
    if variant == "scaled":
        qb.p_scale = torch.tensor([2.0, 0.5, 3.0][:B], dtype=F64, device=device)
        qb.p_diag = torch.tensor([1e-4, 0.0, 5e-5][:B], dtype=F64, device=device)
    return qb


@pytest.mark.parametrize("variant", ["budget", "caps", "lowerside", "scaled", "nobox", "infbox", "perproblem"])
@pytest.mark.parametrize("n", [24, 130, 300])   # below one wave of rows; tails against the 256 stride and the 64 padding
def test_dense_polish_record(device, n, variant):
    qb = _dense_batch(device, n, variant)
    assert qb.shared == (variant != "perproblem") and qb.has_box == (variant != "nobox")
    st = engine.Settings()
    res = engine.solve(qb, st)
    route = f"a k_polish dense n={n} {variant}"
    x, y, zb, status, out = check_records(route, Host(qb), res, st)
    assert np.all(status == _lib.PQ_SOLVED), status
    if variant in ("caps", "perproblem"):
        assert (y[:, 1:] > 0).any(axis=1).all(), y   # a cap binds in every problem
    if variant == "lowerside":
        assert (y[:, 2] < 0).all(), y                # the lower-sided row binds: its gap term is lg y
        assert np.isfinite(out[:, _lib.PQ_OUT_GAP]).all()
    if variant == "infbox":
        third = np.arange(n) % 3
        assert (x[:, third == 0] < 0).any() or (x[:, third == 1] > 0.2).any()   # an infinite side is used
    _report(route)


# ----------------------------------------------------------------------------------------
# b. per-date window polish k_polish_w
# ----------------------------------------------------------------------------------------


DIRECT = ("split", "mixed", "lowerside", "perproblem")   # tests/window_cases.py: the direct capacitance route


def _direct_batch(device, variant, D=6):
    """A 300 x 60 centred window batch whose box rows do not share one rho (or whose rows are per problem),
    with a ridge of 5 % of mean diag P (a unique optimum for the certificate): (case, qb, lr)."""
    kind = "mixed" if variant == "lowerside" else variant
    case = wc.window_case(kind, 300, 60, D, 1, True, 3, ridge=0.05)
    n, t = 300, 100
    if variant == "lowerside":   # budget, a cap, a floor that binds (finite lg, ug = inf) and a two-sided row
        Cg, lg, ug = case["Cg"], case["lg"], case["ug"]
        band = np.zeros((1, 1, n))
        band[0, 0, 2 * t:] = 1.0
        case["Cg"] = np.concatenate([Cg, band], 1)
        case["lg"] = np.concatenate([lg, [[0.10]]], 1)
        case["ug"] = np.concatenate([ug, [[0.40]]], 1)
        case["lg"][0, 2] = 0.45
    if variant == "perproblem":
        # the capped third without its shortable assets (lb = -inf: with them the third's net weight can be cut at
        # no cost and the cap stays slack), capped 0.01 .. 0.02 above what its fixed variables hold: it binds in
        # every problem (checked against the oracle IPM on the CPU: y = 2.6e-4 .. 4.4e-4)
        for c in range(D):
            sup = (case["Cg"][c, 1] > 0) & np.isfinite(case["lb"][c])
            case["Cg"][c, 1] = sup.astype(float)
            case["ug"][c, 1] = case["lb"][c][sup & (case["lb"][c] == case["ub"][c])].sum() + 0.01 + 0.002 * c
    qb, lr, _ = wc.to_device(case, device)
    assert not engine._band_applies(qb, lr)
    return case, qb, lr


def _direct_claims(variant, case, x, y, zb):
    """What makes a direct-route case what it claims to be."""
    c0 = 0
    if variant == "split":
        fixed = case["lb"][c0] == case["ub"][c0]
        assert fixed.any() and (zb[:, fixed] != 0).any(axis=1).all()   # a fixed variable carries a multiplier
        assert np.all(x[:, fixed] == 0.0)
    elif variant == "mixed":
        lo_inf, up_inf = np.isinf(case["lb"][c0]), np.isinf(case["ub"][c0])
        fin_up = case["ub"][c0][~up_inf].max()
        assert (x[:, lo_inf] < 0).any() or (x[:, up_inf] > fin_up).any()   # an infinite side is used
        fixed = case["lb"][c0] == case["ub"][c0]
        assert np.array_equal(x[:, fixed], np.broadcast_to(case["lb"][c0][fixed], x[:, fixed].shape))
    elif variant == "lowerside":
        assert (y[:, 2] < 0).all(), y    # the lower-sided row binds: its gap term is lg y
    elif variant == "perproblem":
        assert (y[:, 1] > 0).all(), y    # a cap binds in every problem


@pytest.mark.parametrize("case", ["centred", "centred_ridge", "uncentred", "relaunch", "woodbury", *DIRECT])
def test_window_polish_record(device, case):
    st, kcap = engine.Settings(), None
    if case in DIRECT:
        host_case, qb, lr = _direct_batch(device, case)
    elif case in ("centred", "centred_ridge"):
        _, _, _, qb, lr = _mv_batch(device, 300, 60, list(range(70, 78)), 0.1, 0.05 if case == "centred_ridge" else 0.0)
    elif case == "uncentred":                       # q = -2 X'y
        qb, lr, _ = grouped_problem(device, 500, 120, 6, 0.1, centred=False)
        st = engine.Settings(rho0_rel=0.5)
    elif case == "relaunch":   # a ridge frees ~120 assets > ldk = 64 < T: overflow, relaunch with ldk = min(ld, 1024)
        _, _, _, qb, lr = _mv_batch(device, 400, 120, [200, 260, 333], 1.0, 2.0)
        kcap = 64
    else:                      # ~115 free assets > ldk = 64 >= T = 60: the first launch solves in Woodbury mode
        _, _, _, qb, lr = _mv_batch(device, 300, 60, list(range(70, 78)), 1.0, 2.0)
        kcap = 64
    ws = engine.Workspace(qb, dense=False, kcap=kcap)
    res = engine.solve_lowrank(qb, lr, st, ws=ws, grouped_polish=False)
    route = f"b k_polish_w {case}"
    x, y, zb, status, out = check_records(route, Host(qb, lr), res, st)
    assert np.all(status == _lib.PQ_SOLVED), status
    if case in DIRECT:
        assert res.capacitance == "direct" and qb.shared == (case != "perproblem")
        _direct_claims(case, host_case, x, y, zb)
    if kcap:
        assert ws.ldk == kcap and out[:, _lib.PQ_OUT_NFREE].min() > kcap, out[:, _lib.PQ_OUT_NFREE]
    _report(route)


# ----------------------------------------------------------------------------------------
# c. grouped pipeline k_pg_post behind its round solvers
# ----------------------------------------------------------------------------------------

TRACKING = dict(rho0_rel=0.1, rho0_qrel=0.0)
GROUPED = {   # name -> (builder, settings overrides, wide_polish)
    "small_T": (lambda d: grouped_problem(d, 300, 60, 40, 1.0), {}, True),
    "capped": (lambda d: grouped_problem(d, 400, 120, 40, 0.05), {}, True),
    "sectors": (lambda d: grouped_problem(d, 600, 150, 36, 0.2, ngroups_rows=5, cap=0.25, stride=2), {}, True),
    "ridge": (lambda d: _with_ridge(grouped_problem(d, 400, 100, 24, 1.0), 5e-3), {}, True),
    # a weaker ridge: free sets of 100..125, the rounds end in the LDS solve k_pg_solve (97..128)
    "ridge_lds": (lambda d: _with_ridge(grouped_problem(d, 400, 100, 24, 1.0), 1.2e-3), {}, True),
    "tracking_ridge": (lambda d: wide_problem(d, 400, 120, 40, -1.0, 1.0, False, ridge=1e-4)[1:], TRACKING, True),
    "tracking_sectors": (lambda d: wide_problem(d, 600, 120, 48, 0.0, 1.0, False, sectors=20, cap=0.15)[1:],
                         TRACKING, True),
    # free sets beyond the K scratch (k > 256): every date is handed back and scored by k_polish_w
    "lsq_handoff": (lambda d: grouped_problem(d, 500, 120, 30, 0.1, centred=False), dict(rho0_rel=0.5), False),
}
THREE_OFF = dict(eps_grouped=0.0, polish_fix_rel=0.0, polish_inner=0)


def _with_ridge(prob, ridge):
    qb, lr, gp = prob
    qb.p_diag = torch.full((qb.batch,), ridge, dtype=F64, device=qb.device)
    return qb, lr, gp


def _bucket(nfree, state, wide):
    if state == _lib.PQ_PG_FALLBACK:
        return "fallback (k_polish_w)"
    if wide:
        return "wide rounds"
    return "register tile <= 96" if nfree <= 96 else ("LDS solve 97..128" if nfree <= 128 else "k_pg_big 129..256")


@functools.lru_cache(maxsize=None)
def _grouped_run(device, case, mode):
    """One grouped solve, checked; returns the bucket of every date (cached: the bucket census re-uses it)."""
    build, over, wide = GROUPED[case]
    qb, lr, gp = build(device)
    st = engine.Settings(**over)
    if mode == "three_off":
        st = dataclasses.replace(st, **THREE_OFF)
    ws = engine.Workspace(qb, dense=False)
    assert engine.grouped_applicable(qb, lr, gp, ws)
    res = engine.solve_lowrank(qb, lr, st, ws=ws, groups=gp, wide_polish=wide)
    torch.cuda.synchronize()
    rec = ws.pg_record().cpu().numpy()
    nfree = res.out[:, _lib.PQ_OUT_NFREE].cpu().numpy()
    buckets = [_bucket(nfree[i], rec[i, _lib.PQ_PG_STATE], rec[i, _lib.PQ_PG_W] == 1.0) for i in range(qb.batch)]
    assert np.all((rec[:, _lib.PQ_PG_STATE] == _lib.PQ_PG_DONE) | (rec[:, _lib.PQ_PG_STATE] == _lib.PQ_PG_FALLBACK))
    _, _, _, status, _ = check_records(f"c {case}", Host(qb, lr), res, st, routes=["c k_pg_post " + b for b in buckets])
    assert np.all(status == _lib.PQ_SOLVED), status
    return tuple(buckets)


@pytest.mark.parametrize("mode", ["default", "three_off"])
@pytest.mark.parametrize("case", list(GROUPED))
def test_grouped_polish_record(device, case, mode):
    buckets = _grouped_run(device, case, mode)
    print(f"[out-record] c {case} {mode}: " + ", ".join(f"{b}: {buckets.count(b)}" for b in sorted(set(buckets))))
    _report("c k_pg_post")


@pytest.mark.parametrize("variant", ["split", "perproblem"])
def test_grouped_polish_record_direct_route(device, variant):
    """The grouped pipeline behind the direct capacitance and the unfused grouped ADMM: fixed split variables
    next to ordinary ones, and per-problem rows and boxes (Cg_stride, g_stride, box_stride != 0)."""
    case, qb, lr = _direct_batch(device, variant)
    gp = engine.GroupPlan(case["rows"], case["tlen"], device)
    st = engine.Settings()
    ws = engine.Workspace(qb, dense=False)
    route = engine.lowrank_route(qb, lr, ws, gp, st)
    assert (route.capacitance, route.admm, route.polish) == ("direct", "grouped-unfused", "grouped")
    res = engine.solve_lowrank(qb, lr, st, ws=ws, groups=gp)
    torch.cuda.synchronize()
    assert res.capacitance == "direct"
    rec = ws.pg_record().cpu().numpy()
    nfree = res.out[:, _lib.PQ_OUT_NFREE].cpu().numpy()
    buckets = [_bucket(nfree[i], rec[i, _lib.PQ_PG_STATE], rec[i, _lib.PQ_PG_W] == 1.0) for i in range(qb.batch)]
    assert np.all((rec[:, _lib.PQ_PG_STATE] == _lib.PQ_PG_DONE) | (rec[:, _lib.PQ_PG_STATE] == _lib.PQ_PG_FALLBACK))
    x, y, zb, status, _ = check_records(f"c direct {variant}", Host(qb, lr), res, st,
                                        routes=[f"c k_pg_post direct {variant} " + b for b in buckets])
    assert np.all(status == _lib.PQ_SOLVED), status
    assert any(b != "fallback (k_polish_w)" for b in buckets), buckets   # k_pg_post scored some date
    _direct_claims(variant, case, x, y, zb)
    print(f"[out-record] c direct {variant}: " + ", ".join(f"{b}: {buckets.count(b)}" for b in sorted(set(buckets))))
    _report(f"c k_pg_post direct {variant}")


def test_grouped_cases_reach_every_scoring_route(device):
    """Across the cases above every bucket is scored at least once: the register-tile solve, k_pg_big with
    state DONE, the hand-off to k_polish_w, the wide rounds and the LDS solve (97..128, the ridge_lds case)."""
    census = {}
    for case in GROUPED:
        for mode in ("default", "three_off"):
            for b in _grouped_run(device, case, mode):
                census[b] = census.get(b, 0) + 1
    msg = f"dates per bucket: {census} (LDS solve 97..128: {census.get('LDS solve 97..128', 0)})"
    print("[out-record] c " + msg)
    for b in ("register tile <= 96", "LDS solve 97..128", "k_pg_big 129..256", "fallback (k_polish_w)", "wide rounds"):
        assert census.get(b, 0) > 0, (b, msg)


# ----------------------------------------------------------------------------------------
# d. ADMM-point scoring (the polish's not-accepted branch; both host repairs off)
# ----------------------------------------------------------------------------------------


def _admm_point_case(device, form):
    if form == "dense":
        qb = _dense_batch(device, 130, "caps")
        return qb, None, lambda st: engine.solve(qb, st)
    _, _, _, qb, lr = _mv_batch(device, 300, 60, list(range(70, 78)), 0.1, 0.0)
    return qb, lr, lambda st: engine.solve_lowrank(qb, lr, st, ws=engine.Workspace(qb, dense=False),
                                                   grouped_polish=False)


@pytest.mark.parametrize("max_iter,expect", [(4000, _lib.PQ_SOLVED_INACCURATE), (5, _lib.PQ_MAX_ITER)])
@pytest.mark.parametrize("form", ["dense", "window"])
def test_admm_point_is_scored_in_place(device, form, max_iter, expect):
    """polish_rounds = 0: no round runs, the kernel scores the ADMM point -- the same x, y, z_box
    bit for bit as a run without any polish, and a record that is true of that point."""
    qb, lr, run = _admm_point_case(device, form)
    st = engine.Settings(polish_rounds=0, refine_retry=1, eps_retry=0.0, max_iter=max_iter)
    r0 = run(dataclasses.replace(st, polish=0))
    torch.cuda.synchronize()
    x0, y0, z0 = (t.cpu().numpy().copy() for t in (r0.x, r0.y, r0.z_box))
    s0 = r0.status.cpu().numpy().copy()
    assert np.all(np.isnan(r0.out[:, :4].cpu().numpy()))          # nothing scored that run
    res = run(st)
    route = f"d ADMM point {form} max_iter={max_iter}"
    x, y, zb, status, out = check_records(route, Host(qb, lr), res, st)
    assert np.all(status == expect), status
    assert np.all(s0 == (_lib.PQ_SOLVED if expect == _lib.PQ_SOLVED_INACCURATE else _lib.PQ_MAX_ITER)), s0
    assert np.array_equal(x, x0) and np.array_equal(y, y0) and np.array_equal(zb, z0)
    assert np.all(out[:, _lib.PQ_OUT_ROUNDS] == 0)
    assert (np.abs(zb) > 0).any() and np.isfinite(out[:, :4]).all()
    _report(route)


# ----------------------------------------------------------------------------------------
# e. pq_polish_lr_batched: k_polish with P x from the window
# ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("setup", ["default", "ridge_refine4"])
def test_polish_lr_batched_record(device, setup):
    """default: P = cov of 60 rows is singular at n = 300 and one refinement step does not settle every date,
    so some polishes are rejected and the kernel scores the ADMM point -- the record must be true of whichever
    point comes back.  ridge_refine4: a ridge and the engine's own repolish setting of 4 refinement steps, so
    that every date is polished on both sides and the comparison of x is one of polished points."""
    n, T, D = 300, 60, 4
    _, _, _, qb, lr = _mv_batch(device, n, T, list(range(70, 70 + D)), 0.1, 0.05 if setup == "ridge_refine4" else 0.0)
    qb.P = lr.panel.cov(lr.rows, lr.tlen, mode=0, mu=lr.mu)        # the same window as a dense matrix
    st = engine.Settings(refine_iters=engine.Settings().refine_retry) if setup == "ridge_refine4" else engine.Settings()
    ws = engine.Workspace(qb)
    engine.solve(qb, dataclasses.replace(st, polish=0), ws=ws)       # K2 + K3 on a fresh workspace
    torch.cuda.synchronize()
    assert bool((ws.status == _lib.PQ_SOLVED).all())
    keep = [ws.x, ws.z, ws.y, ws.status, ws.out]
    saved = [t.clone() for t in keep]
    lib = _lib.load()
    pb, sts, s, l = qb.c_struct(), ws.c_struct(), st.to_c(), lr.c_struct()
    strm = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.pq_polish_batched(ctypes.byref(pb), ctypes.byref(sts), None, 0, ctypes.byref(s), strm),
               "pq_polish_batched")
    torch.cuda.synchronize()
    xd, sd = ws.x[:, :n].cpu().numpy().copy(), ws.status.cpu().numpy().copy()
    for t, v in zip(keep, saved):
        t.copy_(v)
    _lib.check(lib.pq_polish_lr_batched(ctypes.byref(l), ctypes.byref(pb), ctypes.byref(sts), None, 0,
                                        ctypes.byref(s), strm), "pq_polish_lr_batched")
    res = engine._batch_result(qb, ws)
    route = f"e k_polish window P x (pq_polish_lr_batched) {setup}"
    x, y, zb, status, out = check_records(route, Host(qb, lr), res, st)
    print(f"[out-record] e {setup} statuses: pq_polish_batched {sd}, pq_polish_lr_batched {status}")
    assert np.array_equal(sd, status), (sd, status)
    if setup == "ridge_refine4":
        assert np.all(status == _lib.PQ_SOLVED), status
    assert np.abs(x - xd).max() <= 1e-10, np.abs(x - xd).max()
    _report(route)


# ----------------------------------------------------------------------------------------
# f. API level: Solution's numbers are those of its own x, y, z, z_box
# ----------------------------------------------------------------------------------------


def _api_problems(mi, B=3, n=40, nsing=0):
    T = n + 30
    _, R, _, _ = factor_panel(T + 2 * B + 5, n)
    rng = np.random.default_rng(11)
    G = np.zeros((mi, n))
    for r in range(mi):
        G[r, rng.choice(n, size=2 if mi > 3 else n // 3, replace=False)] = 1.0
    h = np.full(mi, 0.12 if mi > 3 else 0.3)
    qps = []
    for i in range(B):
        w = R[5 + 2 * i:5 + 2 * i + T]
        qps.append(QuadraticProgram(P=2.0 * cov_pearson(w), q=-1.0 * w.mean(axis=0), A=np.ones((1, n)), b=np.ones(1),
                                    G=G, h=h, lb=np.zeros(n), ub=np.full(n, 0.2), params={"solver_name": "mi355x"}))
    # singular P (the covariance of 15 rows, rank 14, no linear term): the optimal face is not a point, the
    # interior-point iterate leaves more than 14 assets free and active_set_polish declines (P_FF not PD)
    for i in range(nsing):
        w = R[5 + 2 * i:5 + 2 * i + 15]
        qps.append(QuadraticProgram(P=2.0 * cov_pearson(w), q=np.zeros(n), A=np.ones((1, n)), b=np.ones(1),
                                    G=G, h=h, lb=np.zeros(n), ub=np.full(n, 0.2), params={"solver_name": "mi355x"}))
    return qps


@pytest.mark.parametrize("mi", [3, 70])   # the ADMM route; more than IPM_ROWS rows: the device IPM + active_set_polish
def test_solution_methods_match_an_oracle_solution_of_the_same_point(device, mi):
    from porqua_amd.qp_problems import IPM_ROWS
    qps = _api_problems(mi, nsing=2 if mi == 70 else 0)
    assert (1 + mi > IPM_ROWS) == (mi == 70)
    sols = solve_batch(qps)
    qps[0].solve()
    sols.append(qps[0]["solution"])
    route = f"f API {'IPM route' if mi == 70 else 'ADMM route'}"
    polished = []
    for sol, qp in zip(sols, qps + [qps[0]]):
        assert sol.found and sol.y.shape == (1,) and sol.z.shape == (mi,) and sol.z_box.shape == (40,)
        polished.append(sol.extras.get("active_set_polish"))
        o = OracleSolution(qp["P"], qp["q"], qp["G"], qp["h"], qp["A"], np.atleast_1d(qp["b"]), qp["lb"], qp["ub"])
        o.x, o.y, o.z, o.z_box = sol.x, sol.y, sol.z, sol.z_box
        C, lg, ug = rm.rows_from_qp(o.A, o.b, o.G, o.h, n=40)
        rec = rm.dense_record(o.P, o.q, sol.x, rm.duals_from_qp(sol.y, sol.z), sol.z_box, C=C, lg=lg, ug=ug,
                              lb=o.lb, ub=o.ub)
        eng = {"obj": sol.obj, "prim": sol.primal_residual(), "dual": sol.dual_residual(), "gap": sol.duality_gap()}
        ora = {"obj": o.obj, "prim": o.primal_residual(), "dual": o.dual_residual(), "gap": o.duality_gap()}
        _note(route + (" (polish declined)" if polished[-1] is False else ""), rec,
              {f: rec.units(f, eng[f]) for f in rm.FIELDS})
        for f in rm.FIELDS:
            assert abs(eng[f] - ora[f]) <= rec.bar(f), (route, f, eng[f], ora[f], rec.bar(f))
            assert abs(rm.LD(eng[f]) - rm.LD(rec.value(f))) <= rec.bar(f), (route, f, eng[f], rec.value(f), rec.bar(f))
        assert (sol.z > 0).any()
        if polished[-1] is not False:
            assert sol.is_optimal(1e-7)
    print(f"[out-record] {route}: active_set_polish per problem = {polished}")
    if mi == 70:   # both branches of _solve_batch_ipm are held to the bars: res.Px of a polished and of a declined x
        assert any(p is True for p in polished) and any(p is False for p in polished), polished
    _report(route)


# ----------------------------------------------------------------------------------------
# an unscored point does not read as a perfect one
# ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", ["dense", "window"])
def test_unscored_point_is_not_optimal(device, form):
    """Polish off: nothing scores the ADMM point, so OBJ / PRIM / DUAL / GAP are NaN (not 0) and the
    Solution built from the record is found but not is_optimal()."""
    qb, lr, run = _admm_point_case(device, form)
    if form == "dense":
        res = run(engine.Settings(polish=0))
    else:
        res = engine.solve_lowrank(qb, lr, engine.Settings(), ws=engine.Workspace(qb, dense=False), polish=False)
    torch.cuda.synchronize()
    assert bool((res.status == _lib.PQ_SOLVED).all())
    assert bool(torch.isnan(res.obj).all())
    for sol in batch_result_to_solutions(res, qb):
        assert sol.found and sol.is_optimal() is False and sol.is_optimal(1e9) is False
        for v in (sol.obj, sol.primal_residual(), sol.dual_residual(), sol.duality_gap()):
            assert v != 0 and np.isnan(v)
        assert np.abs(sol.x).max() > 0
