"""tests/residual_model.py (the extended-precision model of the engine's result record) against
the oracle's own residual methods on the golden fixtures, its two forms of P against each other,
infinite and absent bounds, and a sensitivity self-test: the derived bar N u S rejects a P x that
is off by 1e-9 of its size in one entry, which is what a stale vector looks like."""
import numpy as np
import pytest

from oracle.qp_ipm import OracleSolution, solve_qp
from oracle.ref_pipeline import cov_pearson
from porqua_amd.synthetic import factor_panel
from tests import residual_model as rm
from tests.conftest import load_golden


def _oracle_vs_model(P, q, A, b, G, h, lb, ub):
    n = len(q)
    o = solve_qp(P, q, G=G, h=h, A=A, b=b, lb=lb, ub=ub)
    assert o.found
    C, lg, ug = rm.rows_from_qp(o.A, o.b, o.G, o.h, n=n)
    y = rm.duals_from_qp(o.y, o.z)
    assert len(y) == (0 if C is None else C.shape[0])
    rec = rm.dense_record(o.P, o.q, o.x, y, o.z_box, C=C, lg=lg, ug=ug, lb=o.lb, ub=o.ub)
    want = {"obj": o.obj, "prim": o.primal_residual(), "dual": o.dual_residual(), "gap": o.duality_gap()}
    for f in rm.FIELDS:
        assert abs(want[f] - rec.value(f)) <= rec.bar(f), (f, want[f], rec.value(f), rec.bar(f))
    return o, rec


@pytest.mark.parametrize("tag", ["msci_ls", "msci_mv", "msci_qeqw"])
def test_model_matches_the_oracle_on_the_golden_fixtures(tag):
    g = load_golden(tag)
    B = g["P"].shape[0]
    for i in sorted({0, B // 2, B - 1}):
        o, rec = _oracle_vs_model(g["P"][i], g["q"][i], g["A"][i], np.atleast_1d(g["b"][i]), None, None,
                                  g["lb"][i], g["ub"][i])
        assert abs(rec.obj - g["obj"][i]) <= 1e-9 * max(abs(g["obj"][i]), 1e-12)   # the recorded optimum
        assert rec.prim <= 1e-9 and rec.dual <= 1e-9 * max(rec.scale, 1.0)


def test_inequality_multipliers_map_to_the_engine_rows():
    """G x <= h rows follow the equalities with lg = -inf; a binding cap carries z > 0 and enters
    the gap with its ug; the oracle's methods and the model agree on the split."""
    g = load_golden("msci_mv")
    i = 3
    n = g["q"].shape[1]
    x0 = g["x"][i]
    top = np.argsort(-x0)[:3]
    G = np.zeros((2, n))
    G[0, top] = 1.0                       # binding: below what the unconstrained optimum holds there
    G[1, np.argsort(x0)[:5]] = 1.0        # slack
    h = np.array([0.8 * x0[top].sum(), 0.9])
    o, rec = _oracle_vs_model(g["P"][i], g["q"][i], g["A"][i], np.atleast_1d(g["b"][i]), G, h,
                              g["lb"][i], g["ub"][i])
    C, lg, ug = rm.rows_from_qp(o.A, o.b, o.G, o.h, n=n)
    assert C.shape == (3, n) and lg[0] == ug[0] and np.all(np.isinf(lg[1:])) and np.array_equal(ug[1:], h)
    assert o.z[0] > 0 and abs(o.z[1]) <= 1e-12 * abs(o.z[0])
    # the same point with y and z swapped into the wrong rows is not stationary
    wrong = rm.dense_record(o.P, o.q, o.x, np.concatenate([o.z, o.y]), o.z_box, C=C, lg=lg, ug=ug,
                            lb=o.lb, ub=o.ub)
    assert wrong.dual > 1e3 * max(rec.dual, rec.bar("dual"))


def _window_case(n, T, centred, seed=3):
    _, R, yb, _ = factor_panel(T + 9, n)
    X = R[5:5 + T]
    rng = np.random.default_rng(seed)
    x = rng.dirichlet(np.ones(n)) * (rng.random(n) < 0.6)
    x /= x.sum()
    mu = X.mean(axis=0) if centred else None
    q = -0.05 * X.mean(axis=0) if centred else -2.0 * X.T @ yb[5:5 + T]
    C = np.vstack([np.ones(n), (np.arange(n) % 7 == 0).astype(float)])
    lg, ug = np.array([1.0, -np.inf]), np.array([1.0, 0.3])
    y = np.array([-0.37e-3, 0.11e-3])
    lb, ub = np.zeros(n), np.full(n, 0.05)
    z_box = np.where(x == 0, -rng.random(n) * 1e-4, 0.0)
    return X, mu, q, x, y, z_box, C, lg, ug, lb, ub


@pytest.mark.parametrize("n,T", [(300, 60), (130, 40), (600, 150)])
def test_window_form_matches_dense_form(n, T):
    """P = 2 cov_pearson(window) as a dense matrix against the same window in window form: every
    field within the sum of the two bars (the dense side also carries the FP64 rounding of P
    itself, a length-T sum per entry, which the window bar's terms cover)."""
    X, mu, q, x, y, z_box, C, lg, ug, lb, ub = _window_case(n, T, True)
    kw = dict(C=C, lg=lg, ug=ug, lb=lb, ub=ub)
    w = rm.window_record(X, mu, q, x, y, z_box, p_scale=2.0, w_scale=1.0 / (T - 1), p_diag=1e-5, **kw)
    d = rm.dense_record(cov_pearson(X), q, x, y, z_box, p_scale=2.0, p_diag=1e-5, **kw)
    assert w.N == 2 * (n + T + 2 + 16) and d.N == 2 * (n + 2 + 16)
    for f in rm.FIELDS:
        assert abs(w.value(f) - d.value(f)) <= w.bar(f) + d.bar(f), (f, w.value(f), d.value(f), w.bar(f), d.bar(f))
    assert abs(w.scale - d.scale) <= 1e-12 * d.scale
    # uncentred: P = 2 X'X
    X, mu, q, x, y, z_box, C, lg, ug, lb, ub = _window_case(n, T, False)
    w = rm.window_record(X, None, q, x, y, z_box, p_scale=2.0, **kw)
    d = rm.dense_record(X.T @ X, q, x, y, z_box, p_scale=2.0, **kw)
    for f in rm.FIELDS:
        assert abs(w.value(f) - d.value(f)) <= w.bar(f) + d.bar(f), (f, w.value(f), d.value(f))


def test_float64_in_the_kernels_algebra_is_far_inside_the_bar():
    """The kernels' algebra u_t = X_t x - mu x, P x = c (X'u - mu sum u) + p_diag x in plain
    float64 lands within a few u S of the model -- the bar's margin is its N."""
    n, T = 300, 60
    X, mu, q, x, y, z_box, C, lg, ug, lb, ub = _window_case(n, T, True)
    w = rm.window_record(X, mu, q, x, y, z_box, C=C, lg=lg, ug=ug, lb=lb, ub=ub, p_scale=2.0,
                         w_scale=1.0 / (T - 1))
    u = X @ x - mu @ x
    Px = 2.0 * ((1.0 / (T - 1)) * (X.T @ u - mu * u.sum()))
    g = Px + q + C.T @ y + z_box
    assert w.units("dual", float(np.abs(g).max())) <= 16.0
    assert w.units("obj", float(0.5 * x @ Px + q @ x)) <= 16.0
    assert w.N >= 700


def test_infinite_and_absent_bounds_give_finite_results():
    n, T = 130, 40
    X, mu, q, x, y, z_box, C, lg, ug, lb, ub = _window_case(n, T, True)
    lb2, ub2 = lb.copy(), ub.copy()
    lb2[::3] = -np.inf
    ub2[1::3] = np.inf
    lg2, ug2 = np.array([1.0, -np.inf]), np.array([1.0, np.inf])     # a row with no finite side
    for kw in (dict(lb=lb2, ub=ub2, C=C, lg=lg2, ug=ug2), dict(lb=None, ub=None, C=C, lg=lg, ug=ug),
               dict(lb=lb2, ub=None), dict()):
        yy = y if "C" in kw else None
        zz = z_box if kw.get("lb") is not None or kw.get("ub") is not None else None
        for rec in (rm.window_record(X, mu, q, x, yy, zz, p_scale=2.0, w_scale=1.0 / (T - 1), **kw),
                    rm.dense_record(cov_pearson(X), q, x, yy, zz, p_scale=2.0, **kw)):
            for f in rm.FIELDS:
                assert np.isfinite(rec.value(f)) and np.isfinite(rec.bar(f)), (f, kw.keys())
                # (an unconstrained problem has no primal terms: residual and bar are exactly 0)
                assert rec.bar(f) > 0 or (f == "prim" and not kw), (f, kw.keys())
    # an infinite bound contributes nothing to the gap, whatever multiplier sits on it
    a = rm.dense_record(cov_pearson(X), q, x, y, z_box, C=C, lg=lg2, ug=ug2, lb=lb2, ub=ub2)
    zb2 = z_box.copy()
    zb2[::3] = -1.0          # on lb = -inf
    y2 = y.copy()
    y2[1] = 5.0              # on ug = +inf
    b = rm.dense_record(cov_pearson(X), q, x, y2, zb2, C=C, lg=lg2, ug=ug2, lb=lb2, ub=ub2)
    sign = lambda r: float(r.Px @ np.asarray(x, dtype=rm.LD))
    assert sign(a) == sign(b) and abs(a.gap - b.gap) <= a.bar("gap") + b.bar("gap")


@pytest.mark.parametrize("n,T", [(300, 60), (130, 40), (600, 150)])
def test_bar_rejects_a_stale_px_entry(n, T):
    """One entry of P x off by 1e-9 ||P x||inf moves dual or obj outside the bar (and by many bars:
    the bar itself is 1e-13 .. 5e-13 of ||P x||inf on these panels)."""
    X, mu, q, x, y, z_box, C, lg, ug, lb, ub = _window_case(n, T, True)
    kw = dict(C=C, lg=lg, ug=ug, lb=lb, ub=ub)
    w = rm.window_record(X, mu, q, x, y, z_box, p_scale=2.0, w_scale=1.0 / (T - 1), **kw)
    pinf = float(np.abs(w.Px).max())
    assert 1e-14 * pinf <= w.bar("dual") <= 1e-12 * pinf, (w.bar("dual"), pinf)
    Px = np.asarray(w.Px, dtype=np.float64)
    xl = np.asarray(x)
    i = int(np.argmax(xl))                     # a held asset: the entry enters obj and gap too
    Px[i] += 1e-9 * pinf
    g = Px + q + C.T @ y + z_box
    dual = float(np.abs(g).max())
    obj = float(0.5 * xl @ Px + q @ xl)
    miss_dual = abs(dual - w.dual) / w.bar("dual")
    miss_obj = abs(obj - w.obj) / w.bar("obj")
    assert max(miss_dual, miss_obj) > 1.0, (miss_dual, miss_obj)
    # the perturbed component's own stationarity entry is off by thousands of bars
    gi = float(w.Px[i]) + q[i] + C[:, i] @ y + z_box[i]
    assert abs(g[i] - gi) > 1e3 * w.bar("dual")


def test_oracle_solution_round_trip_keeps_the_definitions():
    """OracleSolution filled by hand (as the API-level GPU test does with an engine Solution)
    gives the model's numbers: the two are the same definitions, one in FP64, one extended."""
    n, T = 130, 40
    X, mu, q, x, y, z_box, C, lg, ug, lb, ub = _window_case(n, T, True)
    P = 2.0 * cov_pearson(X)
    o = OracleSolution(P, q, C[1:], ug[1:], C[:1], ug[:1], lb, ub)
    o.x, o.y, o.z, o.z_box = x, y[:1], y[1:], z_box
    rec = rm.dense_record(P, q, x, y, z_box, C=C, lg=lg, ug=ug, lb=lb, ub=ub)
    for f, v in (("obj", o.obj), ("prim", o.primal_residual()), ("dual", o.dual_residual()),
                 ("gap", o.duality_gap())):
        assert abs(v - rec.value(f)) <= rec.bar(f), (f, v, rec.value(f))
