"""tests/admm_reference.py (the dense extended-precision model the ADMM kernels' iterates are
compared with, tests/test_admm_iterates_gpu.py) is itself checked here, without a GPU: run
to convergence it reaches the oracle's optimum, its float64 and longdouble forms agree, and
the Woodbury float64 yardstick is the same iteration."""
import numpy as np

from oracle.qp_ipm import solve_qp
from porqua_amd.synthetic import factor_panel
from tests.admm_reference import LD, admm_dense_ref, admm_woodbury_f64, ref_settings, rel_dist


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
