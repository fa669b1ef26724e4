"""Host-side inputs of the window-form tests on the "direct" capacitance route (TEST
INFRASTRUCTURE ONLY; plain numpy, l1split.split_problem for the split boxes): window batches
whose box rows do not share one ADMM rho, or whose constraints are per problem, so that
engine._band_applies is false and solve_lowrank runs pq_lr_capacitance (k_lr_gram, a per-asset
D) and pq_admm_lr_batched / the unfused pq_admm_lr_grouped.  tests/test_admm_reference.py checks
on the CPU, by the reference alone, the conditions tests/test_window_mixed_gpu.py rests on.

A case is a dict of float64 / int32 host arrays:
    R (rows, n) the panel, rows (B, tmax), tlen (B), mu (B, n) or None (uncentred),
    p_scale, w_scale (B; w_scale None when uncentred), ps = p_scale w_scale, pd (B) or None,
    q (B, n), Cg (nc, mg, n), lg, ug (nc, mg), lb, ub (nc, n) or None, nc = 1 (shared) or B.

Box kinds:
    split       l1split.split_problem of a base problem on n / 2 assets with a sparse previous
                portfolio x0 (about 80 % exactly 0 = lb, two entries exactly at ub = 0.1): the
                variables [u; v] on the panel [R, -R] with the box [0, ub - x0], [0, x0 - lb],
                i.e. fixed [0, 0] rows next to ordinary ones; a transaction cost in q
    mixed       [0, cap] with, at places that differ, ub = 0 (fixed at 0), lb = ub = 0.01 (fixed
                at a non-zero value), ub = inf and lb = -inf (one-sided rows)
    perproblem  shared = False: the mixed box moved and scaled per date, and the budget, the
                caps and Cg itself differ from date to date (box_stride, g_stride, Cg_stride != 0)
    free        the ordinary box with some assets free on both sides (rho_min rows)   } section
    nobox       lb = ub = None                                                         } "free rows"
"""
import numpy as np

from porqua_amd import l1split
from porqua_amd.synthetic import factor_panel
from tests.admm_reference import LD, admm_dense_ref, admm_woodbury_diag_f64

INF = np.inf
KINDS = ("split", "mixed", "perproblem", "free", "nobox")
# The budget row is s 1'x = s with s = 0.25, as in tests/dense_cases.py: its weight rho eq_scale s^2 n
# sets cond(K) and with it the float64 model's distance from the longdouble one.  At s = 1 a single date
# of the uncentred 282 x 150 batch left x at 2.4e-7 (the others 2e-9 .. 5e-8, CPU), no margin under the
# 1e-7 that tests/test_window_mixed_gpu.py needs by the reference alone.
BUDGET_SCALE = 0.25


# The cases of tests/test_window_mixed_gpu.py's iterate tests (and of the CPU conditions in
# tests/test_admm_reference.py): windows n, T, centred, per-date p_diag; every box kind with mg = 1 and 3;
# D = 12 dates at stride 1 and 3 (one group of 12, ragged against admm_grp.hip's GMAX = 16).
WINDOWS = {
    "n282-T150-uncentred": (282, 150, False, False),
    "n282-T20-centred": (282, 20, True, False),
    "n300-T60-centred-pdiag": (300, 60, True, True),
}
DATES = 12
ITER_CASES = [(w, kind, mg, stride) for w in WINDOWS for kind in ("split", "mixed", "perproblem") for mg in (1, 3)
              for stride in (1, 3)]
STOP_CASE = ("n282-T20-centred", "perproblem", 3, 1)
STOP = dict(polish=0, eps_abs=1.6e-3, eps_rel=1.6e-3, eps_grouped=0.0, adapt_interval=0, min_iter=3, max_iter=80)
_GRAMS = {}   # longdouble window Grams, shared by the cases that sit on the same window


def iter_case(window, kind, mg, stride):
    n, T, centred, pdiag = WINDOWS[window]
    return window_case(kind, n, T, DATES, stride, centred, mg, pdiag=pdiag)


def windows(T, D, stride, ragged=False):
    """(rows (D, T) int32, tlen (D,) int32, panel rows needed): D windows of T consecutive panel
    rows, ``stride`` apart; ``ragged``: every third date's window is shorter (T - 1 - 3 (b % 5) rows,
    its list padded with 0 as engine.window_rows pads)."""
    start = 5 + stride * np.arange(D)
    tlen = np.full(D, T, dtype=np.int32)
    if ragged:
        tlen[::3] = T - 1 - 3 * (np.arange(D)[::3] % 5)
    j = np.arange(T)[None, :]
    rows = (start[:, None] + (T - tlen)[:, None] + j) * (j < tlen[:, None])
    return rows.astype(np.int32), tlen, int(start[-1] + T)


def mixed_box(n, nc, cap, free=False):
    """(lb, ub) (nc, n): [0, cap (1 + 0.05 c)]; with i' = i + 3 c: ub = 0 where i' % 11 == 2,
    lb = ub = 0.01 where i' % 13 == 5, ub = inf where i' % 17 == 7, lb = -inf where i' % 7 == 3
    (in that order; an asset that would lose both sides keeps its lower bound).  ``free``: the
    plain box with both sides infinite where i' % 19 == 4 instead."""
    lo, up = np.zeros((nc, n)), np.empty((nc, n))
    for c in range(nc):
        i = np.arange(n) + 3 * c
        up[c] = cap * (1.0 + 0.05 * c)
        if free:
            lo[c, i % 19 == 4], up[c, i % 19 == 4] = -INF, INF
            continue
        up[c, i % 11 == 2] = 0.0
        lo[c, i % 13 == 5] = up[c, i % 13 == 5] = 0.01
        up[c, i % 17 == 7] = INF
        m = (i % 7 == 3) & np.isfinite(up[c]) & (lo[c] < up[c])
        lo[c, m] = -INF
    return lo, up


def portfolio_rows(n, nc, mg):
    """(Cg (nc, mg, n), lg, ug): mg = 1 the budget (equality); mg = 3 plus a cap on the first
    third (one-sided, upper) and a floor on the second (one-sided, lower).  nc > 1: per problem c
    the budget's weights (1, and 1.05 on every 4th asset from c on) and level, the thirds' offsets,
    the cap and the floor differ."""
    assert mg in (1, 3)
    Cg = np.zeros((nc, mg, n))
    lg, ug = np.full((nc, mg), -INF), np.full((nc, mg), INF)
    t = n // 3
    for c in range(nc):
        Cg[c, 0] = BUDGET_SCALE
        if nc > 1:
            Cg[c, 0, c % 4::4] = 1.05 * BUDGET_SCALE
        lg[c, 0] = ug[c, 0] = BUDGET_SCALE * (1.0 - 0.01 * c)
        if mg == 3:
            Cg[c, 1, c:c + t] = 1.0
            ug[c, 1] = 0.30 + 0.02 * c
            Cg[c, 2, t + c:2 * t + c] = 1.0
            lg[c, 2] = 0.10 + 0.005 * c
    return Cg, lg, ug


def kind_rows(n, nc, mg, seed, first=0):
    """Dense random general rows for the capacitance test: row r of problem c is of kind
    (first + r + c) % 4 -- equality, one-sided (upper), two-sided, both bounds infinite."""
    rng = np.random.default_rng(seed)
    Cg = rng.standard_normal((nc, mg, n)) / np.sqrt(n)
    lg, ug = np.full((nc, mg), -INF), np.full((nc, mg), INF)
    v = rng.uniform(0.5, 1.5, size=(nc, mg))
    for c in range(nc):
        for r in range(mg):
            kind = (first + r + c) % 4
            if kind == 0:
                lg[c, r] = ug[c, r] = v[c, r]
            elif kind == 1:
                ug[c, r] = v[c, r]
            elif kind == 2:
                lg[c, r], ug[c, r] = -v[c, r], v[c, r]
    return Cg, lg, ug


def sparse_x0(n0, ub=0.1, seed=7):
    """A long-only previous portfolio on n0 assets: about 80 % of the entries exactly 0, two
    exactly at ``ub``, the rest positive below ub, summing to 0.9 (10 % cash: the split budget row
    then has the right-hand side s 0.1 and the trade must buy.  With a fully invested x0 it is 0,
    nothing of the budget row's weight reaches rhs, and the float64 model sits 1e-14 from the
    longdouble one in x and z: a bar that only the 1e-14 floor decides)."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros(n0)
    held = rng.choice(n0, size=max(4, n0 // 5), replace=False)
    x0[held[:2]] = ub
    w = rng.uniform(0.2, 1.0, size=held.size - 2)
    x0[held[2:]] = (0.9 - 2 * ub) * w / w.sum()
    assert x0.max() <= ub and abs(x0.sum() - 0.9) < 1e-12 and (x0 == 0).mean() > 0.75
    return x0


def window_case(kind, n, T, D=12, stride=1, centred=True, mg=1, pdiag=False, ragged=False, ridge=0.0,
                cap=None):
    """The batch described in the module docstring: D sliding factor_panel windows of T rows on n
    variables (split: n / 2 assets and the panel [R, -R]).

    centred   P_b = p_scale w_scale Xc'Xc (p_scale 2, w_scale 1 / (tlen - 1)), q = -0.05 (window mean)
    else      P_b = 2 X'X, q = -2 X'y (tracking least squares)
    pdiag     a per-date ridge p_diag of 0 .. 5 % of mean diag P;  ridge: the same fraction on every date."""
    assert kind in KINDS and n % 2 == 0
    n0 = n // 2 if kind == "split" else n
    rows, tlen, need = windows(T, D, stride, ragged)
    _, R0, y, _ = factor_panel(need + 2, n0)
    Xs = [R0[rows[b, :tlen[b]]] for b in range(D)]
    mu0 = np.stack([X.mean(0) for X in Xs]) if centred else None
    p_scale = np.full(D, 2.0)
    w_scale = 1.0 / (tlen - 1.0) if centred else None
    ps = p_scale * (w_scale if centred else 1.0)
    Xc = [X - mu0[b] for b, X in enumerate(Xs)] if centred else Xs
    md = np.array([ps[b] * (Xc[b] * Xc[b]).sum(0).mean() for b in range(D)])
    pd = md * np.linspace(0.0, 0.05, D) if pdiag else (md * ridge if ridge else None)
    if centred:
        q0 = -0.05 * mu0
    else:
        q0 = np.stack([-2.0 * X.T @ y[rows[b, :tlen[b]]] for b, X in enumerate(Xs)])
    if kind == "nobox" and centred:
        # without a box a linear term outside range(P) leaves the problem unbounded when p_diag = 0
        # (rank P < T < n): the target-portfolio form q = -P w instead, min (x - w)'P(x - w) on the budget
        w = (1.3 / n0) * (1.0 + 0.5 * np.sin(np.arange(n0)))
        q0 = np.stack([-ps[b] * Xc[b].T @ (Xc[b] @ w) - (pd[b] if pd is not None else 0.0) * w for b in range(D)])
    cap = cap if cap is not None else max(0.2, 8.0 / n0)
    nc = D if kind == "perproblem" else 1
    case = dict(kind=kind, n=n, B=D, centred=centred, rows=rows, tlen=tlen, p_scale=p_scale, w_scale=w_scale,
                ps=ps, pd=pd, nc=nc)
    if kind == "split":
        x0 = sparse_x0(n0)
        Cg0, lg0, ug0 = portfolio_rows(n0, 1, mg)
        # (as l1split.split_batch: the rows and boxes from split_problem with a zero objective)
        base = dict(P=np.zeros((n0, n0)), q=np.zeros(n0), A=Cg0[0, :1], b=lg0[0, :1], lb=np.zeros(n0),
                    ub=np.full(n0, 0.1), G=None, h=None)
        if mg == 3:   # cap: c1 x <= u;  floor: -c2 x <= -l
            base["G"], base["h"] = np.stack([Cg0[0, 1], -Cg0[0, 2]]), np.array([ug0[0, 1], -lg0[0, 2]])
        g0 = np.stack([ps[b] * Xc[b].T @ (Xc[b] @ x0) + (pd[b] if pd is not None else 0.0) * x0 + q0[b]
                       for b in range(D)])
        # a transaction cost below most of |P x0 + q|, so that the optimum trades (at a cost above
        # max|g0| the answer is u = v = 0 and the iteration never leaves the box's corner)
        term = l1split.L1Split("cost", x0, 0.3 * float(np.median(np.abs(g0))))
        sp = l1split.split_problem(base, term)
        C = np.vstack([sp["A"]] + ([sp["G"]] if mg == 3 else []))
        lg = np.concatenate([sp["b"], np.full(mg - 1, -INF)])
        ug = np.concatenate([sp["b"], sp["h"] if mg == 3 else []])
        case.update(R=np.hstack([R0, -R0]), mu=None if mu0 is None else np.hstack([mu0, -mu0]),
                    q=np.hstack([g0 + term.value, -g0 + term.value]), Cg=C[None], lg=lg[None], ug=ug[None],
                    lb=sp["lb"][None], ub=sp["ub"][None], x0=x0)
        fixed = case["lb"] == case["ub"]
        # v is fixed where x0 sits at lb (about 80 % of the assets), u where it sits at ub (two)
        assert fixed[0, :n0].sum() == 2 and fixed[0, n0:].mean() > 0.75 and np.all(np.isfinite(case["ub"]))
    else:
        Cg, lg, ug = portfolio_rows(n, nc, mg)
        if kind == "nobox":
            lb = ub = None
        else:
            lb, ub = mixed_box(n, nc, cap, free=kind == "free")
            both = np.isinf(lb) & np.isinf(ub)
            assert both.any() == (kind == "free")
        case.update(R=R0, mu=mu0, q=q0, Cg=Cg, lg=lg, ug=ug, lb=lb, ub=ub)
    return case


def window_X(case, b):
    """The float64 rows x - mu of problem b, in the kernels' own arithmetic (cached)."""
    cache = case.setdefault("_X", {})
    if b not in cache:
        X = case["R"][case["rows"][b, :case["tlen"][b]]]
        cache[b] = X if case["mu"] is None else X - case["mu"][b]
    return cache[b]


def gram_ld(case, b):
    """Xc'Xc of problem b in longdouble, from float64 rows and means (cached)."""
    rows = case["rows"][b, :case["tlen"][b]]
    key = (case["R"].shape, case["kind"] == "split", case["mu"] is None, rows.tobytes())
    if key not in _GRAMS:
        X = case["R"][rows].astype(LD)
        if case["mu"] is not None:
            X = X - case["mu"][b].astype(LD)
        _GRAMS[key] = X.T @ X
    return _GRAMS[key]


def effective_P(case, b):
    """ps_b Xc'Xc + pd_b I in longdouble."""
    P = LD(case["ps"][b]) * gram_ld(case, b)
    if case["pd"] is not None:
        P[np.diag_indices(case["n"])] += LD(case["pd"][b])
    return P


def initial_rho(case, st):
    """The engine's initial rho on the host: rho0_rel mean diag(P_eff), at least
    rho0_qrel max|q|, clamped (k_init_state with lr.dg, engine._rho_floor_q)."""
    md = np.array([case["ps"][b] * (window_X(case, b) ** 2).sum(0).mean() for b in range(case["B"])])
    if case["pd"] is not None:
        md = md + case["pd"]
    rho = np.clip(st.rho0_rel * md, st.rho_min, st.rho_max)
    return np.clip(np.maximum(rho, st.rho0_qrel * np.abs(case["q"]).max(1)), st.rho_min, st.rho_max)


def problem_args(case, b):
    """(q, Cg, lg, ug, lb, ub) of problem b."""
    c = b % case["nc"]
    return (case["q"][b], case["Cg"][c], case["lg"][c], case["ug"][c],
            None if case["lb"] is None else case["lb"][c], None if case["ub"] is None else case["ub"][c])


def references(case, st, rho, iters=None, model=True, dates=None):
    """(longdouble dense reference, float64 per-asset-D Woodbury model or None) of every problem
    (or of ``dates``) at the initial rho[b], run for ``iters`` iterations (default: to the stop or
    st.max_iter)."""
    ref, mod = [], []
    for b in (range(case["B"]) if dates is None else dates):
        a = problem_args(case, b) + (rho[b], st, iters)
        pd = 0.0 if case["pd"] is None else case["pd"][b]
        ref.append(admm_dense_ref(effective_P(case, b), *a))
        mod.append(admm_woodbury_diag_f64(window_X(case, b), case["ps"][b], *a, p_diag=pd) if model else None)
    return ref, mod


def to_device(case, device):
    """(QPBatch, LowRank, panel) of a case on ``device`` (needs torch and the built library)."""
    import torch
    from porqua_amd import engine
    F64 = torch.float64
    n, B, nc = case["n"], case["B"], case["nc"]
    mg = case["Cg"].shape[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
    qb = engine.QPBatch(n, B, mg, device=device, shared_constraints=nc == 1, has_box=case["lb"] is not None,
                        P=torch.empty(0, dtype=F64, device=device))
    qb.P = None
    ld = qb.ld
    qb.q[:, :n] = t(case["q"])
    qb.Cg[:, :mg, :n] = t(case["Cg"])
    qb.lg[:, :mg], qb.ug[:, :mg] = t(case["lg"]), t(case["ug"])
    if case["lb"] is not None:
        qb.lb[:, n:], qb.ub[:, n:] = 0.0, 0.0   # (the padding, as QPBatch.from_dense leaves it)
        qb.lb[:, :n], qb.ub[:, :n] = t(case["lb"]), t(case["ub"])
    qb.p_scale = t(case["p_scale"])
    qb.p_diag = None if case["pd"] is None else t(case["pd"])
    pan = engine.Panel(case["R"], device=device)
    r_d, t_d = pan.rows_to_device(case["rows"], case["tlen"])
    mu = None
    if case["mu"] is not None:
        mu = torch.zeros((B, ld), dtype=F64, device=device)
        mu[:, :n] = t(case["mu"])
    lr = engine.LowRank(pan, r_d, t_d, mu=mu, w_scale=None if case["w_scale"] is None else t(case["w_scale"]))
    return qb, lr, pan
