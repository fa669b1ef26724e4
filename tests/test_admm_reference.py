"""tests/admm_reference.py (the dense extended-precision model the ADMM kernels' iterates are
compared with, tests/test_admm_iterates_gpu.py) is itself checked here, without a GPU: run
to convergence it reaches the oracle's optimum, its float64 and longdouble forms agree, and
the Woodbury float64 yardstick is the same iteration.  kkt_matrix (the one place the test
side forms K) against a hand-built case, and the dense kernels' float64 yardstick
(admm_explicit_inverse_f64) with the conditions tests/test_dense_admm_iterates_gpu.py rests on."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle.qp_ipm import solve_qp
from porqua_amd.synthetic import factor_panel
from tests import dense_cases, window_cases
from tests.admm_reference import (LD, _iterate, admm_dense_ref, admm_explicit_inverse_f64, admm_woodbury_diag_f64,
                                  admm_woodbury_f64, capacitance_ref, kkt_matrix, ref_settings, rel_dist, row_rho)


def _mean_variance(n, T, lam):
    _, R, _, _ = factor_panel(T + 10, n)
    X = R[5:5 + T]
    Xc = X - X.mean(0)
    ps = 2.0 * lam / (T - 1)
    q = -(np.exp(np.log1p(X).mean(0)) - 1.0)
    Xl = Xc.astype(LD)
    P = LD(ps) * (Xl.T @ Xl)
    rho = max(4.0 * ps * (Xc * Xc).sum(0).mean(), 30.0 * np.abs(q).max())
    return Xc, ps, P, q, rho


def test_reference_converges_to_the_oracle_optimum():
    n, T = 60, 20
    Xc, ps, P, q, rho = _mean_variance(n, T, 5.0)
    Cg = np.zeros((2, n))
    Cg[0] = 1.0
    Cg[1, :n // 3] = 1.0
    lg, ug = np.array([1.0, -np.inf]), np.array([1.0, 0.25])
    lb, ub = np.zeros(n), np.full(n, 0.2)
    st = ref_settings(eps_abs=1e-9, eps_rel=1e-9, adapt_interval=25, max_iter=20000)
    r = admm_dense_ref(P, q, Cg, lg, ug, lb, ub, rho, st)
    assert r.status == "solved" and r.iters < st.max_iter
    P64 = np.asarray(P, dtype=np.float64)
    o = solve_qp(P64, q, G=Cg[1:], h=ug[1:], A=Cg[:1], b=lg[:1], lb=lb, ub=ub)
    assert o.found
    x = np.asarray(r.x, dtype=np.float64)
    f = lambda v: 0.5 * v @ P64 @ v + q @ v
    assert abs(f(x) - f(o.x)) <= 1e-9 * max(1.0, abs(f(o.x))), (f(x), f(o.x))
    assert np.abs(x - o.x).max() <= 1e-6, np.abs(x - o.x).max()
    assert abs(x.sum() - 1.0) <= 1e-8 and x.min() >= -1e-8 and x.max() <= 0.2 + 1e-8
    assert (o.x > 0.2 - 1e-9).any() and (o.x < 1e-9).any()   # both box sides bind at this optimum
    # the last residuals the reference reports are the ones it stopped on
    rp, eps_p, rd, eps_d = r.hist[-1]
    assert rp <= eps_p and rd <= eps_d and len(r.hist) == r.iters


def test_reference_float64_and_longdouble_agree_after_nine_iterations():
    n, T = 60, 20
    st = ref_settings(eps_abs=1e-12, eps_rel=1e-12, adapt_interval=0, max_iter=9)
    lb, ub = np.zeros(n), np.ones(n)
    for lam in (0.1, 10.0):
        Xc, ps, P, q, rho = _mean_variance(n, T, lam)
        for Cg, lg, ug in ((np.ones((1, n)), [1.0], [1.0]), (np.zeros((0, n)), [], [])):
            a = admm_dense_ref(P, q, Cg, lg, ug, lb, ub, rho, st)
            b = admm_dense_ref(np.asarray(P, dtype=np.float64), q, Cg, lg, ug, lb, ub, rho, st, dtype=np.float64)
            w = admm_woodbury_f64(Xc, ps, q, Cg, lg, ug, lb, ub, rho, st)
            assert a.x.dtype == LD and b.x.dtype == np.float64
            assert a.iters == b.iters == w.iters == 9 and a.status == b.status == w.status == "max_iter"
            for k in ("x", "z", "y"):
                assert rel_dist(getattr(b, k), getattr(a, k)) <= 1e-8, (lam, k)
                assert rel_dist(getattr(w, k), getattr(a, k)) <= 1e-6, (lam, k)


def test_reference_adaptive_rho_and_budget():
    """The rho rule is applied at the interval only, an accepted change re-forms K (the next
    residuals move), and an iteration budget below max_iter leaves the problem 'unsolved'."""
    n, T = 60, 20
    Xc, ps, P, q, rho = _mean_variance(n, T, 1.0)
    Cg, lg, ug, lb, ub = np.ones((1, n)), [1.0], [1.0], np.zeros(n), np.ones(n)
    st = ref_settings(eps_abs=1e-12, eps_rel=1e-12, adapt_interval=4, adapt_tol=1.5, max_iter=12)
    a = admm_dense_ref(P, q, Cg, lg, ug, lb, ub, rho, st)
    assert a.iters == 12 and a.status == "max_iter" and len(a.rhos) == 12
    r = [rho] + a.rhos
    assert all(r[i] == r[i - 1] for i in range(1, 13) if i % 4)
    assert r[12] == r[11]   # none at max_iter itself: no iteration would use it
    assert a.rho != rho and st.rho_min <= a.rho <= st.rho_max
    b = admm_dense_ref(P, q, Cg, lg, ug, lb, ub, rho, st, iters=5)
    assert b.iters == 5 and b.status == "unsolved" and b.hist == a.hist[:5]


def test_kkt_matrix_hand_built_rows_of_every_kind():
    """3 x 3, general rows: equality, one-sided, two-sided, unbounded; box: two-sided, fixed, free."""
    inf = np.inf
    P = np.array([[2.0, 0.5, 0.0], [0.5, 3.0, 0.25], [0.0, 0.25, 4.0]])
    Cg = np.array([[1.0, 1.0, 1.0], [1.0, 0.0, 2.0], [0.0, 1.0, -1.0], [3.0, 0.0, 1.0]])
    lg, ug = [1.0, -inf, -0.2, -inf], [1.0, 0.5, 0.3, inf]
    lb, ub = [0.0, 0.1, -inf], [1.0, 0.1, inf]
    st = ref_settings(sigma=1e-3, eq_scale=1e3, rho_min=1e-2)
    rho, eq, mn, sg = 0.5, 0.5 * 1e3, 1e-2, 1e-3
    # P + eq c0 c0' + rho c1 c1' + rho c2 c2' + rho_min c3 c3' (+ sigma + box rho on the diagonal)
    K = np.array([[2.0 + eq + rho * 1.0 + 0.0 + mn * 9.0, 0.5 + eq, 0.0 + eq + rho * 2.0 + mn * 3.0],
                  [0.0, 3.0 + eq + 0.0 + rho * 1.0, 0.25 + eq - rho * 1.0],
                  [0.0, 0.0, 4.0 + eq + rho * 4.0 + rho * 1.0 + mn * 1.0]])
    K = K + np.triu(K, 1).T
    box = np.diag([sg + rho, sg + eq, sg + mn])
    tol = 1e-12   # the expected values are float64 sums of magnitude 1e3; the smallest weight is 1e-2
    for dt in (LD, np.float64):
        got = kkt_matrix(P, Cg, lg, ug, lb, ub, rho, st, dt)
        assert got.dtype == dt and np.abs(got - (K + box)).max() <= tol, np.abs(got - (K + box)).max()
        nobox = kkt_matrix(P, Cg, lg, ug, None, None, rho, st, dt)
        assert np.abs(nobox - (K + sg * np.eye(3))).max() <= tol
        # no general rows: mg = 0
        assert np.array_equal(kkt_matrix(P, np.zeros((0, 3)), [], [], None, None, rho, st, dt),
                              P.astype(dt) + np.diag(np.full(3, dt(sg))))
    # a wrong weight on any kind of row would show: the four kinds' weights all differ
    assert len({eq, rho, mn}) == 3


def test_dense_ref_unchanged_by_kkt_matrix():
    """admm_dense_ref forms K through kkt_matrix: the iterates equal, bit for bit, those of the
    formation it had inline (K = P + Cg' diag(rg) Cg, then sigma + rb on the diagonal)."""
    n, T = 60, 20
    st = ref_settings(eps_abs=1e-12, eps_rel=1e-12, adapt_interval=4, adapt_tol=1.5, max_iter=12)
    Xc, ps, P, q, rho = _mean_variance(n, T, 1.0)
    Cg, lg, ug = np.ones((1, n)), [1.0], [1.0]
    lb, ub = np.zeros(n), np.ones(n)
    ub[3], lb[5], ub[5] = np.inf, -np.inf, np.inf
    Cgd = Cg.astype(LD)

    def inline(rg, rb, rho):
        K = P + Cgd.T @ (rg[:, None] * Cgd)
        K[np.diag_indices(n)] += LD(st.sigma) + rb
        lu = sla.lu_factor(np.asarray(K, dtype=np.float64))

        def solve(rhs):
            x = sla.lu_solve(lu, np.asarray(rhs, dtype=np.float64)).astype(LD)
            for _ in range(3):
                x = x + sla.lu_solve(lu, np.asarray(rhs - K @ x, dtype=np.float64)).astype(LD)
            return x
        return solve

    a = admm_dense_ref(P, q, Cg, lg, ug, lb, ub, rho, st)
    b = _iterate(q, Cg, lg, ug, lb, ub, rho, st, st.max_iter, LD, inline)
    assert a.rho != rho and a.rhos == b.rhos and a.hist == b.hist
    for k in ("x", "z", "y", "Px"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


DENSE_CASES = [(n, c) for n in (24, 130, 300) for c in (True, False)]   # (the larger ones: on the GPU run)


@pytest.mark.parametrize("n,centred", DENSE_CASES)
def test_explicit_inverse_model_distance_and_edges(n, centred):
    """The conditions the dense iterate test rests on, by the reference alone: after 7
    iterations the float64 explicit-inverse model is within 1e-9 of the longdouble model for x,
    z and y (so the 10 d_model bar is never looser than 1e-8; measured <= 4.7e-10 at n <= 130
    and <= 1e-10 beyond) and within 1e-6 for Px (measured <= 2.9e-7); no stop decision of the
    stop-rule run and no accept / reject decision of the adaptive-rho run is within 1e-3 of its
    threshold (measured >= 9.8e-3 and >= 1e-1), and every problem adapts, at iteration 8."""
    from porqua_amd import engine   # (Settings only: host-side defaults of rho0_rel, rho0_qrel)
    case = dense_cases.portfolio_batch(n, 5, centred)
    st = engine.Settings(eps_abs=1e-12, eps_rel=1e-12, adapt_interval=0, max_iter=7)
    rho = dense_cases.initial_rho(case, st)
    assert rho.max() / rho.min() > 1.1
    ref, mod = dense_cases.references(case, st, rho)
    d = {k: max(rel_dist(getattr(m, k), getattr(r, k)) for r, m in zip(ref, mod)) for k in ("x", "z", "y", "Px")}
    print("d_model", n, centred, {k: "%.1e" % v for k, v in d.items()})
    assert all(r.iters == 7 and r.status == "max_iter" for r in ref + mod)
    assert max(d["x"], d["z"], d["y"]) <= 1e-9 and d["Px"] <= 1e-6, d
    st = engine.Settings(eps_abs=1.6e-3, eps_rel=1.6e-3, adapt_interval=0, min_iter=3, max_iter=60)
    ref, _ = dense_cases.references(case, st, rho, model=False)
    assert dense_cases.stop_edge(ref) >= 1e-3 and all(3 <= r.iters < 60 and r.status == "solved" for r in ref)
    st = engine.Settings(eps_abs=1e-12, eps_rel=1e-12, adapt_interval=4, adapt_tol=1.5, max_iter=12)
    ref, mod = dense_cases.references(case, st, rho)
    assert dense_cases.adapt_edge(ref, st) >= 1e-3
    assert all(r.rho != r0 and [c[0] for c in r.cands] == [4, 8] for r, r0 in zip(ref, rho))
    assert max(abs(m.rho / r.rho - 1.0) for r, m in zip(ref, mod)) <= 1e-8


def test_woodbury_diag_model_on_uniform_and_mixed_boxes():
    n, T = 60, 20
    st = ref_settings(eps_abs=1e-12, eps_rel=1e-12, adapt_interval=4, adapt_tol=1.5, max_iter=9)
    Xc, ps, P, q, rho = _mean_variance(n, T, 1.0)
    Cg, lg, ug = np.ones((1, n)), [1.0], [1.0]
    lb, ub = np.zeros(n), np.full(n, 0.2)
    a = admm_woodbury_f64(Xc, ps, q, Cg, lg, ug, lb, ub, rho, st, p_diag=1e-5)
    b = admm_woodbury_diag_f64(Xc, ps, q, Cg, lg, ug, lb, ub, rho, st, p_diag=1e-5)
    assert a.rho != rho and np.allclose(a.rhos, b.rhos, rtol=1e-8, atol=0.0)
    # V V' / d against (V / sqrt(d))(V / sqrt(d))': two roundings of one algebra, each ~1e-8 from the dense model
    # after 9 iterations with two rho changes (y of the budget row is the largest, 3e-9 apart)
    for k in ("x", "z", "y"):
        assert rel_dist(getattr(b, k), getattr(a, k)) <= 1e-7, k
    # fixed at 0 and at a value, a one-sided row of each side: the uniform model refuses, the per-asset one follows
    # the dense model
    ub[3], lb[7], ub[7], ub[11], lb[13] = 0.0, 0.01, 0.01, np.inf, -np.inf
    with pytest.raises(ValueError):
        admm_woodbury_f64(Xc, ps, q, Cg, lg, ug, lb, ub, rho, st)
    Pd = P.copy()
    Pd[np.diag_indices(n)] += LD(1e-5)
    r = admm_dense_ref(Pd, q, Cg, lg, ug, lb, ub, rho, st)
    m = admm_woodbury_diag_f64(Xc, ps, q, Cg, lg, ug, lb, ub, rho, st, p_diag=1e-5)
    assert m.iters == r.iters == 9 and [c[0] for c in m.cands] == [c[0] for c in r.cands] == [4, 8]
    for k in ("x", "z", "y"):
        assert rel_dist(getattr(m, k), getattr(r, k)) <= 1e-8, k
    assert r.z[1 + 3] == 0.0 and r.z[1 + 7] == LD(0.01) and m.z[1 + 3] == 0.0 and m.z[1 + 7] == 0.01   # the fixed rows


def test_capacitance_ref_hand_built():
    """2 window rows padded to tmax = 3, 2 general rows (equality, unbounded), 3 assets: ordinary, fixed, free."""
    inf = np.inf
    st = ref_settings(sigma=1e-3, eq_scale=1e3, rho_min=1e-2)
    X = np.array([[1.0, 2.0, -1.0], [0.5, 0.0, 3.0]])
    Cg = np.array([[1.0, 1.0, 1.0], [2.0, 0.0, -1.0]])
    rho, ps, pdg = 0.5, 4.0, 0.25
    D = np.array([1e-3 + pdg + 0.5, 1e-3 + pdg + 500.0, 1e-3 + pdg + 1e-2])
    U = np.vstack([2.0 * X, np.zeros((1, 3)), np.sqrt(500.0) * Cg[:1], np.sqrt(1e-2) * Cg[1:]])
    want = np.eye(5) + (U / D) @ U.T
    for dt in (LD, np.float64):
        M = capacitance_ref(X, ps, Cg, [1.0, -inf], [1.0, inf], [0.0, 0.1, -inf], [1.0, 0.1, inf], rho, st, p_diag=pdg,
                            tmax=3, dtype=dt)
        assert M.dtype == dt and M.shape == (5, 5) and np.abs(M - want).max() <= 1e-12 * np.abs(want).max()
        assert M[2, 2] == 1.0 and not M[2, :2].any() and not M[2, 3:].any()   # the padding row
        nobox = capacitance_ref(X, ps, Cg, [1.0, -inf], [1.0, inf], None, None, rho, st, p_diag=pdg, tmax=3, dtype=dt)
        assert np.abs(nobox - (np.eye(5) + (U / (1e-3 + pdg)) @ U.T)).max() <= 1e-9 * np.abs(nobox).max()
    assert list(row_rho([0.0, 0.1, -inf], [1.0, 0.1, inf], rho, st)) == [0.5, 500.0, 1e-2]


@pytest.mark.parametrize("window,kind,mg,stride", window_cases.ITER_CASES)
def test_direct_route_model_distance(window, kind, mg, stride):
    """The conditions tests/test_window_mixed_gpu.py::test_direct_route_iterates rests on, by the reference
    alone: after 7 iterations the float64 per-asset-D Woodbury model is within 1e-7 of the longdouble model for
    x, z and y on every case (so the 10 d_model bar is never looser than 1e-6) and never closer than 1e-13 (so the
    1e-14 floor decides nothing).  Measured, worst over the 12 dates: split x 2.9e-11 .. 9.2e-11, z 5.0e-12 ..
    4.3e-10, y 4.2e-10 .. 9.4e-10, Px 3.8e-9 .. 2.1e-8; mixed and perproblem x 1.9e-11 .. 3.1e-9, z 7.2e-12 ..
    2.2e-9, y 3.5e-10 .. 1.4e-9, Px 1.7e-8 .. 7.8e-8 (the uncentred 282 x 150 windows the largest in x)."""
    from porqua_amd import engine   # (Settings only: host-side defaults of rho0_rel, rho0_qrel)
    case = window_cases.iter_case(window, kind, mg, stride)
    st = engine.Settings(polish=0, eps_abs=1e-12, eps_rel=1e-12, adapt_interval=0, max_iter=7)
    rho = window_cases.initial_rho(case, st)
    ref, mod = window_cases.references(case, st, rho, 7)
    d = {k: max(rel_dist(getattr(m, k), getattr(r, k)) for r, m in zip(ref, mod)) for k in ("x", "z", "y", "Px")}
    print("d_model", window, kind, mg, stride, {k: "%.1e" % v for k, v in d.items()})
    assert all(r.iters == 7 and r.status == "max_iter" for r in ref + mod)
    assert 10.0 * max(d["x"], d["z"], d["y"]) <= 1e-6 and min(d.values()) >= 1e-13, d
    fixed = case["lb"] == case["ub"]
    assert fixed.any() and not fixed.all() and (case["nc"] > 1) == (kind == "perproblem")


def test_direct_route_stop_and_adapt_edges():
    """The one stop-count case (282 x 20 centred, per-problem rows, mg = 3) by the reference alone: with eps
    1.6e-3, min_iter 3 no residual / eps ratio of any iteration is within 1e-3 of 1 (measured 1.18e-2; 40 .. 50
    iterations); with interval 4, tol 1.5 every problem adapts at iterations 4 and 8, no candidate is within 1e-3 of
    its threshold (measured 2.2e-1) and the model's rho is within 1e-8 of the reference's (2.2e-9)."""
    from porqua_amd import engine
    case = window_cases.iter_case(*window_cases.STOP_CASE)
    st = engine.Settings(**window_cases.STOP)
    rho = window_cases.initial_rho(case, st)
    ref, _ = window_cases.references(case, st, rho, model=False)
    edge = dense_cases.stop_edge(ref)
    its = [r.iters for r in ref]
    print("stop edge %.2e iterations %d..%d" % (edge, min(its), max(its)))
    assert edge >= 1e-3 and all(r.status == "solved" for r in ref)
    assert min(its) >= st.min_iter and max(its) < st.max_iter and len(set(its)) > 4
    st = engine.Settings(polish=0, eps_abs=1e-12, eps_rel=1e-12, adapt_interval=4, adapt_tol=1.5, max_iter=12)
    ref, mod = window_cases.references(case, st, rho)
    assert dense_cases.adapt_edge(ref, st) >= 1e-3
    assert all(r.rho != r0 and [c[0] for c in r.cands] == [4, 8] for r, r0 in zip(ref, rho))
    assert max(abs(m.rho / r.rho - 1.0) for r, m in zip(ref, mod)) <= 1e-8
