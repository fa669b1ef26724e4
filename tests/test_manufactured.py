"""The conditions tests/test_polish_buckets_gpu.py rests on, by the reference alone (CPU): every
manufactured optimum of tests/manufactured.py is a KKT point at rounding level, unique (reduced
Hessian positive definite on the active rows' null space, strictly complementary multipliers,
x*_F well inside the box), the float64 yardstick reduced_kkt_f64 started 1e-7 away lands within
the 1e-9 its bar is designed to stay under, and the engine's algorithm restated in numpy
(tests/engine_model.py) recovers F and x* from its own ADMM stop.

The batches of tests/test_polish_per_date_gpu.py (manufactured.PER_DATE) meet the same conditions; their
start point (manufactured.start_state) is classified by start_box / start_row exactly as constructed,
the yardstick of each batch's mode stays under the design bar, and every date of the flip batches has
a wrongly classified start from which the numpy model of the polish ends on (F, active rows) in 2 or 3
rounds.  d_model reached from the 1e-7 start, worst over x and the multipliers -- one step on every
date, with refine_iters = 1 and with refine_retry = 4 alike (the stop rule ends the refinement after
it); every batch with a ridge of 4 x mean diag P, chosen here and not from a GPU number:
  compact   cA 4.1e-15  cT20 1.3e-15  cT32 1.4e-15  cT33 1.1e-15  cT65 1.3e-15  cB 6.6e-16  cW 9.0e-16
            cR16 2.4e-15  cR32 1.3e-15  cN 2.7e-15  cBig 4.7e-15  fA 5.3e-15  eC 9.0e-16  (oA within these)
  Woodbury  wA 4.9e-15  wW 3.8e-15  wT64 4.9e-15  wT60 5.1e-15  wT65 5.3e-15  wN 3.4e-15  wC8 2.7e-15
            fW 4.6e-15  eW 2.5e-15
  dense     dA 4.5e-15  dN 9.2e-16  dA1024 4.3e-14  dC8 4.5e-15  dU 5.3e-15"""
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


# the batches of tests/test_polish_per_date_gpu.py (manufactured.PER_DATE); see the module docstring

FAMILY_A_Q_SHA256 = "91d138f15e826d972fa798ea72115c5dd148effcae3534231181fd409ab1c356"


def test_family_a_inputs_are_bit_for_bit_what_they_were():
    """family() grew (n, T, sizes, ridge) arguments; the q of family A with the defaults is the one the
    grouped solvers' tests have always been given."""
    import hashlib
    q = np.stack([o.q for o in batch("A").opt])
    assert q.shape == (48, 300) and hashlib.sha256(q.tobytes()).hexdigest() == FAMILY_A_Q_SHA256


@functools.lru_cache(maxsize=None)
def pbatch(name):
    return mf.per_date(name)


@pytest.mark.parametrize("name", list(mf.PER_DATE))
def test_per_date_points_are_unique_kkt_points(name):
    b = pbatch(name)
    n = b.n
    eq = b.lg == b.ug
    box = bool(np.isfinite(b.lb).all())
    for d, o in enumerate(b.opt):
        x, lam, z = (v.astype(np.float64) for v in (o.x, o.lam, o.z))
        r = kkt_residuals(b.P64(d), o.q, x, A=b.C[eq] if eq.any() else None, b=b.ug[eq] if eq.any() else None,
                          G=b.C[~eq] if (~eq).any() else None, h=b.ug[~eq] if (~eq).any() else None,
                          lb=b.lb if box else None, ub=b.ub if box else None,
                          y=np.concatenate([lam[eq], lam[~eq]]), z_box=z)
        m = o.margins
        assert m["kkt_res"] <= 1e-17, (name, d, m)
        # float64 evaluation of an n-term stationarity sum: n u of the gradient scale (1e-13 at n = 300)
        tol = 1e-13 * max(n, 300) / 300
        assert r["stat"] <= tol and r["comp"] <= tol and r["dual"] == 0.0 and r["prim"] <= 1e-14, (name, d, r)
        assert len(o.F) == b.sizes[d] and np.all(o.side[o.F] == 0) and o.p_diag > 0.0
        assert m["z_min_rel"] >= 0.4 and m["moved"] <= 1e-11, (name, d, m)
        assert np.all(o.z[o.F] == 0) and np.all(o.lam[~o.act] == 0)
        if o.k == 0:      # the multiplier of a row without free support is not unique: nothing more to ask
            assert name == "cK0" or name == "dA"
            continue
        assert m["lam_min"] > 0.0 and m["lam_min_rel"] >= 1e-4, (name, d, m)
        assert m["row_min_rel"] >= 0.4 and m["slack_min"] >= 0.04 and m["gap"] >= m["gap_need"], (name, d, m)
    mas = sorted(set(int(o.act.sum()) for o in b.opt))
    assert mas == [{"N": 0, "R16": 17, "R32": 33, "C8": 9}.get(b.fam, 1)], (name, mas)
    if b.fam in ("B", "W"):
        assert all(np.any(np.where(o.side == 1, b.lb, b.ub)[o.side != 0] != 0.0) for o in b.opt if o.k < n)   # nzb


@pytest.mark.parametrize("flip", [None, "fix", "free"])
@pytest.mark.parametrize("name", list(mf.PER_DATE))
def test_start_state_is_classified_as_constructed(name, flip):
    """start_box / start_row (polish_rules.h, restated in manufactured.rule_start_*) return side and the active
    rows exactly from start_state -- but for the one flipped variable."""
    b = pbatch(name)
    mg = b.C.shape[0]
    for d, o in enumerate(b.opt):
        if flip and (o.k == 0 or o.k == b.n or not np.isfinite(b.lb).all()):   # nothing to flip
            continue
        x, z, y, i = mf.start_state(b, d, flip=flip)
        side = mf.rule_start_box(z[mg:], y[mg:], x, b.lb, b.ub)
        act = mf.rule_start_row(z[:mg], y[:mg], b.lg, b.ug)
        want = o.side.copy()
        if flip == "fix":
            assert o.side[i] == 0
            want[i] = 1
        elif flip == "free":
            assert o.side[i] != 0
            want[i] = 0
        assert np.array_equal(side, want), (name, d, np.flatnonzero(side != want))
        assert np.array_equal(act != 0, o.act) and np.all(act[o.act] == 2), (name, d, act)
        assert np.abs(x - o.x.astype(np.float64)).max() <= 1e-7 * float(np.abs(o.x).max())
        assert np.array_equal(x[o.side != 0], np.where(o.side == 1, b.lb, b.ub)[o.side != 0])


@pytest.mark.parametrize("refine", [1, REFINE_RETRY])
@pytest.mark.parametrize("name", list(mf.PER_DATE))
def test_per_date_yardstick_stays_under_its_design_bar(name, refine):
    """10 d_model <= 1e-9 from the 1e-7 start, with the yardstick of the batch's mode (compact and dense:
    reduced_kkt_f64; Woodbury: reduced_kkt_woodbury_f64, which takes max(refine, 2) steps at most) and the
    refinement counts the kernel is run with."""
    b = pbatch(name)
    mg = b.C.shape[0]
    worst = 0.0
    for d, o in enumerate(b.opt):
        if o.k == 0:
            continue
        x0, _, y0, _ = mf.start_state(b, d)
        (x, lam, zb, steps), _ = mf.per_date_model(b, d, x0, y0[:mg], DELTA, refine)
        assert 1 <= steps <= (max(refine, 2) if b.mode == "woodbury" else refine)
        dx = float(np.abs(x - o.x).max() / np.abs(o.x).max())
        dm = float(max(np.abs(lam - o.lam).max(initial=0.0), np.abs(zb - o.z).max()) / o.s)
        worst = max(worst, dx, dm)
        assert 10.0 * max(dx, dm) <= 1e-9, (name, d, o.k, dx, dm)
    print(f"[manufactured] {name} ({b.mode}, refine {refine}): worst d_model over x and the multipliers {worst:.2e}")


def test_woodbury_yardstick_is_the_compact_one_in_another_algebra():
    """Both yardsticks solve the same regularised system: from the same start they agree far inside the bar."""
    b = pbatch("wC8")
    mg = b.C.shape[0]
    for d, o in enumerate(b.opt):
        x0, _, y0, _ = mf.start_state(b, d)
        X, mu = b.X(d), b.mu[d]
        sc = mf.problem_scale(X, mu, b.psw(d), o.p_diag, o.q)
        args = (X, mu, b.psw(d), o.p_diag, o.q, b.C, b.lg, b.ug, b.lb, b.ub, o.side, o.act, x0, y0[:mg], DELTA * sc, 2)
        xa, la, za, _ = mf.reduced_kkt_f64(*args)
        xw, lw, zw, _ = mf.reduced_kkt_woodbury_f64(*args)
        assert np.abs(xa - xw).max() <= 1e-13 * np.abs(xa).max()
        assert max(np.abs(la - lw).max(), np.abs(za - zw).max()) <= 1e-13 * o.s


@pytest.mark.parametrize("refine", [1, REFINE_RETRY])
@pytest.mark.parametrize("name", [k for k, c in mf.PER_DATE.items() if c.get("flip")])
def test_flipped_starts_end_on_the_optimum_in_the_models_rounds(name, refine):
    """Every date of the flip batches has a wrongly classified start from which the numpy model of the
    engine's polish ends at (F, active rows) in 2 .. polish_rounds rounds: that count is what the kernel's
    PQ_OUT_ROUNDS is held to."""
    b = pbatch(name)
    steps = max(refine, 2) if b.mode == "woodbury" else refine
    got = [mf.flip_start(b, d, delta=DELTA, dual_tol=1e-9, rounds=8, refine=steps) for d in range(b.D)]
    assert all(g is not None for g in got), (name, [g is not None for g in got])
    print(f"[manufactured] {name} refine {refine}: (k, flipped variable, kind, model rounds) "
          f"{[(o.k,) + g[3:] for o, g in zip(b.opt, got)]}")
    assert {g[4] for g in got} == {"fix", "free"} and all(2 <= g[5] <= 8 for g in got)
