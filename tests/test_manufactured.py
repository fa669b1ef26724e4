"""The conditions tests/test_polish_buckets_gpu.py rests on, by the reference alone (CPU): every
manufactured optimum of tests/manufactured.py is a KKT point at rounding level, unique (reduced
Hessian positive definite on the active rows' null space, strictly complementary multipliers,
x*_F well inside the box), the float64 yardstick reduced_kkt_f64 started 1e-7 away lands within
the 1e-9 its bar is designed to stay under, and the engine's algorithm restated in numpy
(tests/engine_model.py) recovers F and x* from its own ADMM stop."""
import functools
import os
import re

import numpy as np
import pytest

from tests import manufactured as mf
from tests.engine_model import admm, polish
from tests.kkt import kkt_residuals

DELTA = 1e-9         # engine.Settings.delta
REFINE_RETRY = 4     # engine.Settings.refine_retry


@functools.lru_cache(maxsize=None)
def batch(fam):
    return mf.family(fam)


def _p64(b, d):
    o = b.opt[d]
    return mf.window_P(b.X(d), None if b.mu is None else b.mu[d], b.psw(d), o.p_diag).astype(np.float64)


@pytest.mark.parametrize("fam", mf.FAMILIES)
def test_manufactured_points_are_kkt_points(fam):
    b = batch(fam)
    eq = b.lg == b.ug
    worst = dict(stat=0.0, prim=0.0, dual=0.0, comp=0.0)
    for d, o in enumerate(b.opt):
        x, lam, z = (v.astype(np.float64) for v in (o.x, o.lam, o.z))
        r = kkt_residuals(_p64(b, d), o.q, x, A=b.C[eq], b=b.ug[eq], G=b.C[~eq] if (~eq).any() else None,
                          h=b.ug[~eq] if (~eq).any() else None, lb=b.lb, ub=b.ub,
                          y=np.concatenate([lam[eq], lam[~eq]]), z_box=z)
        for f in worst:
            worst[f] = max(worst[f], r[f])
        assert o.margins["kkt_res"] <= 1e-17, (fam, d, o.margins)   # the longdouble solve itself
    print(f"[manufactured] {fam}: kkt residuals of (x*, lambda, z) in float64: {worst}")
    # float64 evaluation of an n = 300 stationarity sum: n u of the gradient scale
    assert worst["stat"] <= 1e-13 and worst["comp"] <= 1e-13 and worst["dual"] == 0.0, worst
    assert worst["prim"] <= 1e-14, worst


@pytest.mark.parametrize("fam", mf.FAMILIES)
def test_manufactured_optima_are_unique_and_inside_the_box(fam):
    b = batch(fam)
    keys = ("lam_min_rel", "cond", "z_min_rel", "row_min_rel", "slack_min", "gap", "moved")
    for d, o in enumerate(b.opt):
        m = o.margins
        print(f"[manufactured] {fam} date {d:2d} k {o.k:3d} ma {int(o.act.sum())} p_diag {o.p_diag:.2e}  "
              + "  ".join(f"{k} {m[k]:.2e}" for k in keys))
        assert len(o.F) == b.sizes[d] and np.all(o.side[o.F] == 0)
        assert (o.p_diag == 0.0) == (d < b.nplain)
        assert m["lam_min"] > 0.0 and m["lam_min_rel"] >= 1e-4, (fam, d, m)     # unique
        assert m["z_min_rel"] >= 0.4 and m["row_min_rel"] >= 0.4, (fam, d, m)  # strictly complementary
        assert m["slack_min"] >= 0.04, (fam, d, m)                             # inactive rows stay inactive
        assert m["gap"] >= m["gap_need"], (fam, d, m)                          # x*_F inside the box
        assert m["moved"] <= 1e-11, (fam, d, m)                                # rounding q moved x* by ~cond u
        assert np.all(o.z[o.F] == 0) and np.all(o.lam[~o.act] == 0)
    if fam == "B":   # pass 0 is live on every date
        assert all((o.side == 2).sum() >= 2 for o in b.opt)
    if fam.startswith("C"):
        assert all(int(o.act.sum()) == 1 + int(fam[1:]) for o in b.opt)
    if fam == "W":
        assert sorted(set(b.n - o.k for o in b.opt)) == list(mf.W_FIXED)


@pytest.mark.parametrize("fam", mf.FAMILIES)
def test_float64_yardstick_stays_under_its_design_bar(fam):
    """10 d_model <= 1e-9 for every date, from a start 1e-7 (relative) away from the optimum -- the stop of
    the tight mode's ADMM -- with at most refine_retry refinement steps and the kernels' residual test:
    the tight bar of the GPU test is never looser than 1e-9."""
    b = batch(fam)
    rng = np.random.default_rng(5)
    worst = 0.0
    for d, o in enumerate(b.opt):
        X, mu = b.X(d), None if b.mu is None else b.mu[d]
        x0 = o.x.astype(np.float64) + 1e-7 * np.abs(o.x).max().astype(np.float64) * rng.uniform(-1, 1, b.n)
        l0 = o.lam.astype(np.float64) * (1.0 + 1e-7 * rng.uniform(-1, 1, len(o.lam)))
        sc = mf.problem_scale(X, mu, b.psw(d), o.p_diag, o.q)
        x, lam, zb, steps = mf.reduced_kkt_f64(X, mu, b.psw(d), o.p_diag, o.q, b.C, b.lg, b.ug, b.lb, b.ub, o.side,
                                               o.act, x0, l0, DELTA * sc, REFINE_RETRY, stop=mf.STOP_REL * sc)
        assert 1 <= steps <= REFINE_RETRY
        dx = float(np.abs(x - o.x).max() / np.abs(o.x).max())
        dm = float(max(np.abs(lam - o.lam).max(), np.abs(zb - o.z).max()) / o.s)
        worst = max(worst, dx, dm)
        assert 10.0 * max(dx, dm) <= 1e-9, (fam, d, o.k, dx, dm)
    print(f"[manufactured] {fam}: worst d_model over x and the multipliers {worst:.2e}")


@pytest.mark.parametrize("fam", mf.FAMILIES)
def test_stop_rule_keeps_the_tight_bar_under_its_design_value(fam):
    """By the reference alone and from any starting point: whatever iterate the kernels' stop rule admits is
    within 1e-10 of (x*, lambda, z) on every date that meets the tight bar, so 10 d_model <= 1e-9 there.
    (The ridge of a family is the lever: manufactured.RIDGE.)"""
    b = batch(fam)
    worst = [0.0, 0.0]
    for d, o in enumerate(b.opt):
        if not mf.in_tight_bar(fam, o):
            continue
        X, mu = b.X(d), None if b.mu is None else b.mu[d]
        bx, bm = mf.stop_rule_bound(_p64(b, d), o.q, b.C, b.lg, b.ug, o, mf.problem_scale(X, mu, b.psw(d), o.p_diag, o.q))
        worst = [max(worst[0], bx), max(worst[1], bm)]
        assert 10.0 * bx <= 1e-9 and 10.0 * bm <= 1e-9, (fam, d, o.k, bx, bm)
    print(f"[manufactured] {fam}: stop-rule bound on d_model, worst x {worst[0]:.1e} multipliers {worst[1]:.1e}")
    assert (worst[0] > 0.0) == (fam not in ("C8", "W"))


# one small instance per family: (family, date) -- a ridged free set beyond the register tile where the
# family has one
MODEL_CASES = [("A", 3), ("A", 29), ("B", 1), ("B", 9), ("C1", 3), ("C8", 5), ("W", 5)]


@pytest.mark.parametrize("fam,d", MODEL_CASES)
def test_engine_model_recovers_the_free_set(fam, d):
    b = batch(fam)
    o = b.opt[d]
    n = b.n
    P = _p64(b, d)
    C = np.vstack([b.C, np.eye(n)])
    l = np.concatenate([np.where(np.isfinite(b.lg), b.lg, -1e30), b.lb])
    u = np.concatenate([np.where(np.isfinite(b.ug), b.ug, 1e30), b.ub])
    sc = max(np.abs(o.q).max(), np.abs(np.diag(P)).max())
    r = admm(P, o.q, C, l, u, rho=4.0 * np.mean(np.diag(P)), scaling=0, eps_abs=1e-7, eps_rel=1e-7, max_iter=20000)
    assert r["status"] == "solved", r["iters"]
    x, lam, zb, rounds, ok = polish(P, o.q, C, l, u, r["x"], r["y"], r["z"], delta=DELTA * sc, dual_tol=1e-9 * sc)
    free = np.flatnonzero((x > b.lb) & (x < b.ub))
    err = float(np.abs(x - o.x).max() / np.abs(o.x).max())
    print(f"[manufactured] model {fam} date {d} k {o.k}: ADMM {r['iters']} iterations, {rounds} polish rounds, "
          f"|x - x*| / |x*| {err:.2e}")
    assert ok and np.array_equal(free, o.F), (rounds, len(free), o.k)
    assert np.array_equal(np.flatnonzero(zb == 0.0), o.F)
    assert err <= 1e-9, err
    assert np.abs(lam - o.lam).max() <= 1e-9 * o.s and np.abs(zb - o.z).max() <= 1e-9 * o.s


def test_the_kernels_rules_header_states_the_models_constants():
    """The constants every polish kernel takes from porqua_amd/csrc/polish_rules.h are the ones this
    model states (STOP_REL, ROW_ZERO), read from the header itself; the inner step's box tolerance is 1e-12."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "porqua_amd", "csrc",
                        "polish_rules.h")
    found = dict(re.findall(r"^constexpr double (POLISH_\w+) = ([0-9.eE+-]+);", open(path).read(), flags=re.M))
    assert set(found) == {"POLISH_STOP_REL", "POLISH_ROW_ZERO", "POLISH_INNER_BOX_TOL"}, found
    assert float(found["POLISH_STOP_REL"]) == mf.STOP_REL
    assert float(found["POLISH_ROW_ZERO"]) == mf.ROW_ZERO
    assert float(found["POLISH_INNER_BOX_TOL"]) == 1e-12
