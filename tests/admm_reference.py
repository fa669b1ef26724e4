"""Dense extended-precision model of the window-form ADMM kernels' iteration (TEST
INFRASTRUCTURE ONLY; plain numpy / scipy, nothing of the engine is imported).

The low-rank ADMM entry points (pq_admm_lr_batched, pq_admm_lr_grouped, pq_admm_lr_gcap,
pq_admm_lr_sweep) all run the unscaled OSQP iteration on

    min 0.5 x'Px + q'x   s.t.  lg <= Cg x <= ug,  lb <= x <= ub

with the rows C = [Cg; I], a per-row rho (rho, rho * eq_scale on equality rows, rho_min on
rows without bounds) and K = P + sigma I + C' diag(rv) C:

    rhs = sigma x - q + C'(rv * z - y)           x~ = K^-1 rhs           z~ = C x~
    Px~ = rhs - sigma x~ - C'(rv * z~)
    x  <- alpha x~  + (1 - alpha) x              Px <- alpha Px~ + (1 - alpha) Px
    z^ =  alpha z~  + (1 - alpha) z
    z  <- clip(z^ + y / rv, l, u)                y  <- y + rv * (z^ - z)

from x = Px = z = y = 0, with the stop  rp = max|Cx - z| <= eps_abs + eps_rel max(|Cx|, |z|)
and  rd = max|Px + q + C'y| <= eps_abs + eps_rel max(|Px|, |C'y|, |q|)  from ``min_iter``
on, OSQP's adaptive rho every ``adapt_interval`` iterations (accepted outside ``adapt_tol``,
K re-formed; not at ``max_iter`` itself, where the run ends and a new rho would serve no
iteration) and status 'max_iter' at ``max_iter``.

``admm_dense_ref`` is that iteration for one problem with K solved densely -- in
np.longdouble by default: K is factored in float64 (LAPACK has no extended precision) and
every solve takes three steps of iterative refinement on longdouble residuals.
``admm_woodbury_f64`` is the same iteration in float64 through the kernels' own algebra,
K^-1 = (I - V' M^-1 V / d) / d with an explicit inverse of the capacitance M = I + V V' / d.
Its distance from the dense model measures the rounding that algebra amplifies: it is the
yardstick of tests/test_admm_iterates_gpu.py and nothing else; ``admm_woodbury_diag_f64`` is the
same for box rows that do not share one rho (a per-asset D; tests/test_window_mixed_gpu.py), and
``capacitance_ref`` the capacitance M = I + U D^-1 U' itself.  ``admm_explicit_inverse_f64``
plays the same role for the dense kernels (pq_factor_batched + pq_admm_batched,
tests/test_dense_admm_iterates_gpu.py): float64 with an explicit K^-1 = L^-T L^-1.
``kkt_matrix`` is the one place K is formed (also the reference of
tests/test_kkt_factor_gpu.py).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

LD = np.longdouble

_DEFAULTS = dict(sigma=1e-6, alpha=1.6, eps_abs=2e-3, eps_rel=2e-3, rho_min=1e-6, rho_max=1e6,
                 adapt_tol=5.0, eq_scale=1e3, max_iter=4000, adapt_interval=60, min_iter=0)


def ref_settings(**kw):
    """The settings the iteration reads (any object with these attributes will do)."""
    bad = set(kw) - set(_DEFAULTS)
    if bad:
        raise TypeError(f"unknown settings {sorted(bad)}")
    return SimpleNamespace(**{**_DEFAULTS, **kw})


def row_rho(l, u, rho, st):
    """Per-row rho: rho * eq_scale on equality rows, rho_min on rows without bounds."""
    l, u = np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)
    return np.where(l == u, rho * st.eq_scale, np.where(np.isinf(l) & np.isinf(u), st.rho_min, rho))


def _amax(*vs):
    return max((float(np.abs(v).max()) for v in vs if v.size), default=0.0)


def _iterate(q, Cg, lg, ug, lb, ub, rho, st, iters, dt, make_solver):
    """The iteration itself; make_solver(rg, rb, rho) -> (rhs -> K^-1 rhs) for the current rho
    (rg, rb: its per-row values)."""
    n = q.shape[0]
    Cg = np.asarray(Cg, dtype=dt).reshape(-1, n)
    mg = Cg.shape[0]
    q = np.asarray(q, dtype=dt)
    lg, ug = np.asarray(lg, dtype=np.float64).reshape(mg), np.asarray(ug, dtype=np.float64).reshape(mg)
    lb, ub = np.asarray(lb, dtype=np.float64).reshape(n), np.asarray(ub, dtype=np.float64).reshape(n)
    lgd, ugd, lbd, ubd = (a.astype(dt) for a in (lg, ug, lb, ub))
    sigma, alpha = dt(st.sigma), dt(st.alpha)
    rho = float(rho)

    def rows(rho):
        rg, rb = row_rho(lg, ug, rho, st).astype(dt), row_rho(lb, ub, rho, st).astype(dt)
        return rg, rb, make_solver(rg, rb, rho)

    rg, rb, solve = rows(rho)
    x, Px, zb, yb = (np.zeros(n, dt) for _ in range(4))
    zg, yg = np.zeros(mg, dt), np.zeros(mg, dt)
    qmax = _amax(q)
    hist, rhos, cands, it, status = [], [], [], 0, "unsolved"
    end = min(int(iters), int(st.max_iter))
    while it < end:
        it += 1
        rhs = sigma * x - q + Cg.T @ (rg * zg - yg) + (rb * zb - yb)
        xt = solve(rhs)
        ztg = Cg @ xt
        pxt = rhs - sigma * xt - Cg.T @ (rg * ztg) - rb * xt
        x = alpha * xt + (1 - alpha) * x
        Px = alpha * pxt + (1 - alpha) * Px
        zhg = alpha * ztg + (1 - alpha) * zg
        zhb = alpha * xt + (1 - alpha) * zb
        zgn = np.clip(zhg + yg / rg, lgd, ugd)
        zbn = np.clip(zhb + yb / rb, lbd, ubd)
        yg = yg + rg * (zhg - zgn)
        yb = yb + rb * (zhb - zbn)
        zg, zb = zgn, zbn
        cgx = Cg @ x
        cty = Cg.T @ yg + yb
        rp = _amax(cgx - zg, x - zb)
        rd = _amax(Px + q + cty)
        sp = _amax(cgx, x, zg, zb)
        sd = max(_amax(Px, cty), qmax)
        eps_p = st.eps_abs + st.eps_rel * sp
        eps_d = st.eps_abs + st.eps_rel * sd
        hist.append((rp, eps_p, rd, eps_d))
        if it >= st.min_iter and rp <= eps_p and rd <= eps_d:
            status = "solved"
            break
        if st.adapt_interval > 0 and it % st.adapt_interval == 0 and it < st.max_iter:
            rn = rho * np.sqrt((rp / (sp + 1e-30)) / (rd / (sd + 1e-30) + 1e-30))
            rn = min(max(float(rn), st.rho_min), st.rho_max)
            cands.append((it, rn, rho))
            if rn > rho * st.adapt_tol or rn < rho / st.adapt_tol:
                rho = rn
                rg, rb, solve = rows(rho)
        rhos.append(rho)
        if it >= st.max_iter:
            status = "max_iter"
    return SimpleNamespace(x=x, z=np.concatenate([zg, zb]), y=np.concatenate([yg, yb]), Px=Px, iters=it,
                           status=status, rho=rho, hist=hist, rhos=rhos, cands=cands)


def kkt_matrix(P, Cg, lg, ug, lb, ub, rho, settings, dtype=LD):
    """K = P + sigma I + Cg' diag(rg) Cg + diag(rb) in ``dtype`` for an effective P (the one
    place the test side forms it): rg / rb = row_rho of the general / box rows.  ``lb`` None:
    no box rows."""
    dt = np.dtype(dtype).type
    P = np.asarray(P, dtype=dt)
    n = P.shape[0]
    Cgd = np.asarray(Cg, dtype=dt).reshape(-1, n)
    mg = Cgd.shape[0]
    rg = row_rho(np.reshape(lg, mg), np.reshape(ug, mg), rho, settings).astype(dt)
    K = P + Cgd.T @ (rg[:, None] * Cgd)
    d = dt(settings.sigma)
    if lb is not None:
        d = d + row_rho(np.reshape(lb, n), np.reshape(ub, n), rho, settings).astype(dt)
    K[np.diag_indices(n)] += d
    return K


def admm_dense_ref(P, q, Cg, lg, ug, lb, ub, rho, settings=None, iters=None, dtype=LD):
    """``iters`` iterations (default: until the stop or max_iter) of the ADMM above for one
    problem, K solved densely in ``dtype`` (np.longdouble or np.float64).  Returns x, z and y
    (rows [general; box]), Px, iters, status ('solved', 'max_iter', 'unsolved': the budget
    ran out), the final rho, ``hist``: (rp, eps_p, rd, eps_d) of every iteration, ``rhos``: the
    rho after every iteration that did not stop, and ``cands``: (iteration, candidate rho, rho
    before) of every adaptive-rho decision.

    P may be given in ``dtype`` already (form it once per date and scale it per problem: an
    extended-precision n^3 product per problem is slow)."""
    st = settings or ref_settings()
    dt = np.dtype(dtype).type
    P = np.asarray(P, dtype=dt)
    n = P.shape[0]
    Cgd = np.asarray(Cg, dtype=dt).reshape(-1, n)

    def make_solver(rg, rb, rho):
        K = kkt_matrix(P, Cgd, lg, ug, lb, ub, rho, st, dt)
        lu = sla.lu_factor(np.asarray(K, dtype=np.float64))
        if dt is np.float64:
            return lambda rhs: sla.lu_solve(lu, rhs)

        def solve(rhs):
            x = sla.lu_solve(lu, np.asarray(rhs, dtype=np.float64)).astype(dt)
            for _ in range(3):
                r = rhs - K @ x
                x = x + sla.lu_solve(lu, np.asarray(r, dtype=np.float64)).astype(dt)
            return x
        return solve

    return _iterate(np.asarray(q), Cg, lg, ug, lb, ub, rho, st, st.max_iter if iters is None else iters, dt,
                    make_solver)


def admm_woodbury_f64(Xc, ps, q, Cg, lg, ug, lb, ub, rho, settings=None, iters=None, p_diag=0.0):
    """The same iteration in float64 through the kernels' algebra, for P = ps Xc'Xc + p_diag I
    and a box whose rows all take one rho (d = sigma + p_diag + rho_box):
    V = [sqrt(ps) Xc; sqrt(rg) Cg], M = I + V V' / d, explicit inv(M),
    x~ = (rhs - V' M^-1 V rhs / d) / d."""
    st = settings or ref_settings()
    Xc = np.asarray(Xc, dtype=np.float64)
    n = Xc.shape[1]
    Cgd = np.asarray(Cg, dtype=np.float64).reshape(-1, n)

    def make_solver(rg, rb, rho):
        if not np.all(rb == rb[0]):
            raise ValueError("admm_woodbury_f64: the box rows must share one rho")
        dinv = 1.0 / (st.sigma + p_diag + rb[0])
        V = np.vstack([np.sqrt(ps) * Xc, np.sqrt(rg)[:, None] * Cgd])
        Minv = np.linalg.inv(np.eye(V.shape[0]) + (V @ V.T) * dinv)
        return lambda rhs: (rhs - V.T @ (Minv @ (V @ (rhs * dinv)))) * dinv

    return _iterate(np.asarray(q), Cg, lg, ug, lb, ub, rho, st, st.max_iter if iters is None else iters,
                    np.float64, make_solver)


def admm_woodbury_diag_f64(Xc, ps, q, Cg, lg, ug, lb, ub, rho, settings=None, iters=None, p_diag=0.0):
    """admm_woodbury_f64 for box rows that do NOT share one rho (a fixed variable, a free one or
    an infinite side among ordinary ones; the kernels' "direct" capacitance, k_lr_gram): the
    per-asset D = sigma + p_diag + rb, W = V diag(1 / sqrt(D)), M = I + W W', explicit inv(M),
    x~ = D^-1 (rhs - V' M^-1 V D^-1 rhs).  The yardstick of tests/test_window_mixed_gpu.py."""
    st = settings or ref_settings()
    Xc = np.asarray(Xc, dtype=np.float64)
    n = Xc.shape[1]
    Cgd = np.asarray(Cg, dtype=np.float64).reshape(-1, n)

    def make_solver(rg, rb, rho):
        dinv = 1.0 / (st.sigma + p_diag + rb)
        V = np.vstack([np.sqrt(ps) * Xc, np.sqrt(rg)[:, None] * Cgd])
        W = V * np.sqrt(dinv)
        Minv = np.linalg.inv(np.eye(V.shape[0]) + W @ W.T)
        return lambda rhs: (rhs - V.T @ (Minv @ (V @ (rhs * dinv)))) * dinv

    return _iterate(np.asarray(q), Cg, lg, ug, lb, ub, rho, st, st.max_iter if iters is None else iters,
                    np.float64, make_solver)


def capacitance_ref(Xc, ps, Cg, lg, ug, lb, ub, rho, settings=None, p_diag=0.0, tmax=None, dtype=LD):
    """M = I + U D^-1 U' of one problem as lowrank.hip's header defines it, in ``dtype``:
    U = [sqrt(ps) Xc (padded with zero rows to ``tmax``); sqrt(rg) Cg], k = tmax + mg rows,
    D = sigma + p_diag + rb per asset (rb = 0 for a batch without a box, lb None); rg / rb =
    row_rho.  Xc is taken as given (float64: the centring x - mu is the kernel's own input
    arithmetic and is done by the caller in float64, as the kernel does it)."""
    st = settings or ref_settings()
    dt = np.dtype(dtype).type
    Xc = np.asarray(Xc, dtype=np.float64)
    T, n = Xc.shape
    tmax = T if tmax is None else int(tmax)
    Cgd = np.asarray(Cg, dtype=np.float64).reshape(-1, n)
    mg = Cgd.shape[0]
    rg = row_rho(np.reshape(lg, mg), np.reshape(ug, mg), rho, st)
    D = np.full(n, dt(st.sigma) + dt(p_diag))
    if lb is not None:
        D = D + row_rho(np.reshape(lb, n), np.reshape(ub, n), rho, st).astype(dt)
    U = np.zeros((tmax + mg, n), dtype=dt)
    U[:T] = np.sqrt(dt(ps)) * Xc.astype(dt)
    U[tmax:] = np.sqrt(rg.astype(dt))[:, None] * Cgd.astype(dt)
    return np.eye(tmax + mg, dtype=dt) + (U / D) @ U.T


def admm_explicit_inverse_f64(P, q, Cg, lg, ug, lb, ub, rho, settings=None, iters=None):
    """The same iteration in float64 through the dense kernels' algebra (pq_factor_batched with
    an inverse, then k_admm's symmetric mat-vec): K = L L' by numpy.linalg.cholesky,
    K^-1 = L^-T L^-1 formed explicitly from inv(L), x~ = K^-1 rhs."""
    st = settings or ref_settings()
    P = np.asarray(P, dtype=np.float64)

    def make_solver(rg, rb, rho):
        Li = np.linalg.inv(np.linalg.cholesky(kkt_matrix(P, Cg, lg, ug, lb, ub, rho, st, np.float64)))
        Kinv = Li.T @ Li
        return lambda rhs: Kinv @ rhs

    return _iterate(np.asarray(q), Cg, lg, ug, lb, ub, rho, st, st.max_iter if iters is None else iters,
                    np.float64, make_solver)


def rel_dist(a, ref):
    """max|a - ref| / max|ref| (1 when ref is zero and a is not)."""
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    sc = float(np.abs(ref).max()) if ref.size else 0.0
    d = float(np.abs(a - ref).max()) if ref.size else 0.0
    return d / sc if sc > 0.0 else (0.0 if d == 0.0 else 1.0)
