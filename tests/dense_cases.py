"""Host-side inputs of the dense-path tests (TEST INFRASTRUCTURE ONLY; plain numpy): general
rows and boxes with one row of every kind the kernels tell apart, and the portfolio batches of
tests/test_dense_admm_iterates_gpu.py.  tests/test_admm_reference.py checks on the CPU, by the
reference alone, the conditions those GPU tests rest on.

Row kinds (rho_for in chol_dev.h, rho_row in admm.hip): equality (lg == ug: rho eq_scale),
one-sided and two-sided (rho), both bounds infinite (rho_min)."""
import numpy as np

from porqua_amd.synthetic import factor_panel
from tests.admm_reference import LD, admm_dense_ref, admm_explicit_inverse_f64

INF = np.inf


def general_rows(n, mg, nc, seed):
    """(Cg (nc, mg, n), lg, ug (nc, mg)): row r is of kind r % 4 -- equality, one-sided (upper
    bound only), two-sided, both bounds infinite; nc > 1: rows and bounds that differ between the
    problems.  Dense random coefficients (a matrix test; see portfolio_rows for the ADMM runs)."""
    rng = np.random.default_rng(seed)
    Cg = rng.standard_normal((nc, mg, n)) / np.sqrt(n)
    lg, ug = np.full((nc, mg), -INF), np.full((nc, mg), INF)
    v = rng.uniform(0.5, 1.5, size=(nc, mg))
    for r in range(mg):
        kind = r % 4
        if kind == 0:
            lg[:, r] = ug[:, r] = v[:, r]
        elif kind == 1:
            ug[:, r] = v[:, r]
        elif kind == 2:
            lg[:, r], ug[:, r] = -v[:, r], v[:, r]
    return Cg, lg, ug


def mixed_box(n, nc, ub=0.2):
    """(lb, ub) of shape (nc, n): ordinary bounds [0, ub (1 + 0.1 c)], and per problem c (at
    places that move with c) a fixed variable (lb == ub), a free one (both infinite) and a
    one-sided one (no upper bound)."""
    lo = np.zeros((nc, n))
    up = np.empty((nc, n))
    for c in range(nc):
        up[c] = ub * (1.0 + 0.1 * c)
        i = (3 + 5 * c) % n
        lo[c, i] = up[c, i] = 0.01
        lo[c, (i + 7) % n], up[c, (i + 7) % n] = -INF, INF
        up[c, (i + 12) % n] = INF
    return lo, up


def portfolio_rows(n, nc):
    """(Cg (nc, 4, n), lg, ug): the budget s 1'x = s (equality), a cap on the first third
    (one-sided), a band on the second third (two-sided) and a row without bounds (rho_min) --
    per problem c the caps, the band and the thirds' offsets differ.

    s = 1 up to 130 assets and 0.25 beyond: the budget row's weight rho eq_scale s^2 n sets
    cond(K) ~ eq_scale s^2 n, and with it the distance of the float64 explicit-inverse model
    from the longdouble one (about 10 cond(K) eps after 7 iterations).  At s = 1 that distance
    was 3.5e-10 .. 6.3e-10 at n = 130 and 4.5e-10 .. 1.2e-9 at 300, 520 and 900 (CPU, over window
    lengths and BLAS thread counts): no margin under the 1e-9 that
    tests/test_dense_admm_iterates_gpu.py needs by the reference alone.  With s = 0.25 the
    larger sizes stay below 1e-10."""
    s = 1.0 if n <= 130 else 0.25
    Cg = np.zeros((nc, 4, n))
    lg, ug = np.full((nc, 4), -INF), np.full((nc, 4), INF)
    t = n // 3
    for c in range(nc):
        o = c % max(t, 1)
        Cg[c, 0] = s
        lg[c, 0] = ug[c, 0] = s
        Cg[c, 1, o:o + t] = 1.0
        ug[c, 1] = 0.30 + 0.02 * c
        Cg[c, 2, t:2 * t + o] = 1.0
        lg[c, 2], ug[c, 2] = 0.10 + 0.01 * c, 0.45 - 0.01 * c
        Cg[c, 3, ::2] = 1.0
        Cg[c, 3, 1::2] = -1.0 - 0.1 * c
    return Cg, lg, ug


def portfolio_batch(n, B, centred, T=None, stride=5):
    """B problems from sliding factor_panel windows of T rows (default 60):

    centred   P_b = the window's covariance, a small linear q = -0.05 (window mean), shared
              rows and box                                   (mean-variance with little return)
    else      P_b = X'X, q = -2 p_scale X'y of the tracking least squares, per-problem rows
              and boxes

    p_scale (1.6 .. 2.4) and p_diag (a 0 .. 5 % ridge of mean diag P) vary over the batch.
    Returns a dict of float64 host arrays: P (B, n, n), ps, pd, q (B, n), Cg (nc, 4, n), lg, ug,
    lb, ub (nc, n)."""
    T = T or 60
    _, R, y, _ = factor_panel(T + stride * (B - 1), n)
    X = np.stack([R[b * stride:b * stride + T] for b in range(B)])
    Y = np.stack([y[b * stride:b * stride + T] for b in range(B)])
    ps = np.linspace(1.6, 2.4, B) if B > 1 else np.array([2.0])
    nc = 1 if centred else B
    if centred:
        mu = X.mean(1, keepdims=True)
        X = X - mu
        w = 1.0 / (T - 1)
        q = -0.05 * mu[:, 0, :]
    else:
        w = 1.0
        q = -2.0 * ps[:, None] * np.einsum("bti,bt->bi", X, Y)
    P = w * np.einsum("bti,btj->bij", X, X)
    md = np.einsum("bii->b", P) / n
    pd = md * np.linspace(0.0, 0.05, B)
    Cg, lg, ug = portfolio_rows(n, nc)
    lb, ub = mixed_box(n, nc, ub=max(0.2, 4.0 / n))
    return dict(n=n, B=B, P=P, ps=ps, pd=pd, q=q, Cg=Cg, lg=lg, ug=ug, lb=lb, ub=ub)


def initial_rho(case, st):
    """The engine's initial rho on the host: rho0_rel mean diag(ps P + pd I), at least
    rho0_qrel max|q|, clamped (k_init_state, engine._rho_floor_q)."""
    md = case["ps"] * np.einsum("bii->b", case["P"]) / case["n"] + case["pd"]
    rho = np.clip(st.rho0_rel * md, st.rho_min, st.rho_max)
    return np.clip(np.maximum(rho, st.rho0_qrel * np.abs(case["q"]).max(1)), st.rho_min, st.rho_max)


def effective_P(case, b):
    """ps_b P_b + pd_b I of problem b in longdouble, from the float64 P_b the kernels are given (cached)."""
    cache = case.setdefault("_P", {})
    if b not in cache:
        P = LD(case["ps"][b]) * case["P"][b].astype(LD)
        P[np.diag_indices(case["n"])] += LD(case["pd"][b])
        cache[b] = P
    return cache[b]


def references(case, st, rho, model=True):
    """(longdouble reference, float64 explicit-inverse model or None) of every problem of the
    batch at the initial rho[b], run to the stop or st.max_iter."""
    nc = case["Cg"].shape[0]
    ref, mod = [], []
    for b in range(case["B"]):
        c = b % nc
        a = (case["q"][b], case["Cg"][c], case["lg"][c], case["ug"][c], case["lb"][c], case["ub"][c], rho[b], st)
        P = effective_P(case, b)
        ref.append(admm_dense_ref(P, *a))
        mod.append(admm_explicit_inverse_f64(np.asarray(P, dtype=np.float64), *a) if model else None)
    return ref, mod


def stop_edge(ref):
    """The nearest any iteration's rp / eps_p or rd / eps_d comes to 1, over the batch."""
    return min(min(abs(rp / ep - 1.0), abs(rd / ed - 1.0)) for r in ref for rp, ep, rd, ed in r.hist)


def adapt_edge(ref, st):
    """The nearest any adaptive-rho candidate comes to the accept / reject thresholds
    rho adapt_tol and rho / adapt_tol (relative), over the batch."""
    return min(min(abs(rn / (rho * st.adapt_tol) - 1.0), abs(rn * st.adapt_tol / rho - 1.0))
               for r in ref for _, rn, rho in r.cands)
