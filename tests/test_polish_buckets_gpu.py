"""The grouped polish's round solvers on manufactured optima (tests/manufactured.py): problems
whose optimum x*, multipliers and free set F are known by construction, so the free-set size k
is an input of the test and only the end state is compared -- with x* itself, not with another
kernel or an oracle solve.  Everything goes through engine.solve_lowrank with a GroupPlan on
consecutive daily windows, n = 300 (ld 320), T = 120:

  family A   centred, box [0, 1], budget: one batch of 48 dates, k = 2, 15, 16, 17, 47, 48, 49, 63, 64,
             65, 79, 80, 81, 95, 96, 97, 127, 128, 129, 200, 255, 256, 257, 299, each twice: every
             edge of rt_solve_date<3..6> (k <= 48 / 64 / 80 / 96), the LDS k_pg_solve (97..128),
             k_pg_big (129..256) and the hand-off to the per-date k_polish_w beyond PG_KBIG = 256
  family B   centred, box [0, 0.05], weights at the upper bound (x_B != 0: pass 0 is live),
             k = 30, 48, 49, 64, 96, 97, 128, 200
  family C   budget + 10 disjoint sector caps with 1, 7 and 8 of them active: ma = 2, 8, 9 active
             rows straddle RT_WMA = WMA = 8 of the register, LDS and big solves; k = 40, 64, 90, 120.
             With 9 active rows k_pg_setup keeps the date (ma <= PG_MGMAX = 32) and the round's solver
             hands it back (state FALLBACK): the per-date kernel is the intended route
  family W   uncentred (the tracking form), box [-1, 1], ridge, budget; n - k = 0, 3, 7, 8 variables at
             a bound: 1, 4 and 8 bordered rows take the wide rounds (polish_gw.hip, PG_WMB = 8), 9 do
             not, and with k = 292 > PG_KBIG that date is handed to the per-date kernel

No ridge up to k = 49 (A) / k <= T / 2 (B, C), one ridge per batch beyond (manufactured.RIDGE x
mean diag P of its ridged dates; see below).
The dates without a ridge come first and the GroupPlan breaks there, so every group has one
p_diag and the batch keeps the group capacitance (asserted); the plan is built for one CU, so
family A's polish groups hold 14 + 2 + 16 + 16 dates and its group-capacitance groups 14 + 10 + 24.

Two settings modes.  tight: eps_grouped = 0, polish_fix_rel = 0, polish_inner = 0, eps 1e-7 -- the
ADMM identifies F, so the last round is the one solve of size k_d on the solver k_d selects --
with the default refine_iters and with refine_iters = refine_retry.  default: engine.Settings()
as shipped (loose 7-iteration stop, polish_fix_rel, polish_inner, several rounds, growing and
shrinking free lists).

Bars.  (a) exact: status SOLVED, PQ_OUT_NFREE = k_d, {i: lb < x_i < ub} = F, z_box zero exactly
there; tight mode also the record state (DONE with R_KB = k_d, or FALLBACK), PQ_PG_W, and the
solver census.  (b) the standing parity bars of tests/test_headline_parity_gpu.py against x*:
weights 1e-5 L-inf, objective 1e-6 relative, violation 1e-7, plus the certificate bars of
tests/test_polish_wide_gpu.py (workloads.window_certificate), every family and mode.  (c) tight
mode with refine_retry steps, the register-tile, LDS and k_pg_big solvers, per date:

    |x - x*|inf / |x*|inf  <=  10 d_model + 1e-14,    the same for (lambda, z_box) relative to s

with d_model the same distance for the float64 yardstick manufactured.reduced_kkt_f64 started
from the kernel's own ADMM point (read back from a run without polish), and 10 d_model <= 1e-9
asserted (tests/test_manufactured.py bounds d_model by the reference alone, from any starting
point).  The wide rounds keep (b): their algebra (a group capacitance at delta_wide) has no
float64 model here yet.  The per-date kernel keeps (b) in this file and is held to (c), in its
compact and its Woodbury mode, by tests/test_polish_per_date_gpu.py.

Two properties of the kernels' algorithm had to be restated in the yardstick and in the
problems, neither fitted to a measured number:
  * every polish kernel ends its refinement once the residual of the regularised system is
    within 1e-13 of the problem scale (row residuals within 1e-14 (1 + |d_a| + |C_aF x_F|) count as
    zero).  Without that rule the yardstick refines on to cond(P_FF) u, 4e-16 .. 5e-15, while
    the solvers, by design, stop after the one step that takes the eps = 1e-7 ADMM point
    (1e-5 .. 2e-1 from x*, relative) to 4e-15 .. 4e-10: ratios of 143 and 413 on the first dates
    compared (k = 2 and 40, rt<3>).  With the rule the yardstick takes the same steps (one; two
    at k = 200) and agrees with every solver to two digits: a property of the algorithm, the
    same in polish.hip, polish_w.hip, k_pg_solve, k_pg_big and rt_solve_date, and no defect;
  * from such an ADMM point the one step left d_model = 3.6e-10 at k = 255 with the ridge of 0.05
    mean diag P, so 10 d_model <= 1e-9 did not hold by the reference alone.  The ridge is the
    lever: 4 / 1 / 1 x mean diag P for A / B / C (manufactured.RIDGE), where the largest error the
    stop rule admits from ANY start is <= 9.7e-11 (manufactured.stop_rule_bound).  W keeps 0.05.

Measured on an MI355X.  Tight mode, both refine settings: every date SOLVED in one round on the
solver its k selects, ADMM 41 .. 422 iterations; dates per solver
  A    rt<3> 12, rt<4> 6, rt<5> 6, rt<6> 6, LDS 97..128 6, k_pg_big 8, per-date fallback 4
  B    rt<3> 4, rt<4> 4, rt<6> 2, LDS 97..128 4, k_pg_big 2
  C1   rt<3> 2, rt<4> 2, rt<6> 2, LDS 97..128 2            C7   the same
  C8   per-date fallback 8                                  W    wide 6, per-date fallback 2
worst |x - x*|inf 5.0e-14 (A), 7.3e-14 (B), 8.1e-14 (C1), 5.0e-14 (C7), 7.7e-15 (C8), 1.6e-12 (W);
objective <= 1.9e-15 relative, violation <= 8.9e-16, certificate stationarity <= 2.4e-14.
Default mode: 7 .. 33 ADMM iterations, 1 .. 7 rounds, 0 .. 8 dates per batch handed to the per-date
kernel; worst |x - x*|inf 6.2e-10 (A), 2.3e-10 (B), 1.6e-10 (C1), 1.4e-10 (C7), 4.6e-16 (C8), 3.9e-13 (W),
objective <= 1.0e-11, violation <= 8.1e-12, certificate stationarity <= 3.4e-10.
Bar (c), worst d_kernel / d_model per solver (d_kernel / d_model of that date):
                 x                              multipliers
  rt<3>          1.06  (8.7e-14 / 8.3e-14)      1.08  (7.0e-15 / 6.5e-15)
  rt<4>          1.09  (2.3e-14 / 2.1e-14)      1.09  (2.5e-15 / 2.3e-15)
  rt<5>          0.94  (1.5e-15 / 1.6e-15)      1.14  (2.3e-15 / 2.0e-15)
  rt<6>          1.08  (1.4e-15 / 1.3e-15)      2.22  (9.5e-16 / 4.3e-16)
  LDS 97..128    1.26  (1.8e-15 / 1.5e-15)      1.87  (7.9e-16 / 4.2e-16)
  k_pg_big       1.09  (5.8e-15 / 5.3e-15)      2.44  (6.6e-16 / 2.7e-16)
No solver missed a bar and no kernel was changed.  What the bar sees: a build whose
rt_solve_date<5> returns its fourth free weight off by 1e-9 relative fails bar (c) on the six
rt<5> dates of family A (d_kernel 6.4e-10 against d_model 1.2e-15) and passes the rest of this
file and tests/test_polish_grouped_gpu.py.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.workloads import window_certificate
from tests import manufactured as mf

pytestmark = pytest.mark.gpu
F64 = torch.float64
LD = np.longdouble

TIGHT = dict(eps_grouped=0.0, polish_fix_rel=0.0, polish_inner=0, eps_abs=1e-7, eps_rel=1e-7)
R_KB = 349            # pg_record.h: the free-set size k_pg_setup found this round
RT_WMA = 8            # polish_rt.hip / polish_g.hip: active general rows of a round's solve
SOLVERS = ("rt<3>", "rt<4>", "rt<5>", "rt<6>", "LDS 97..128", "k_pg_big", "wide", "per-date fallback")
MODELLED = SOLVERS[:6]
RATIOS = {}           # solver -> [worst d_kernel / d_model, worst d_kernel, its d_model] (bar c)


def _expected(fam, k, ma, nfx):
    """The solver the code intends for a final round of free-set size k with ma active rows and nfx variables
    at a bound (k_pg_setup, pg_bucket, the solvers' ma > 8 hand-off; ldk = 256 at n = 300)."""
    if fam == "W" and k > 128 and ma + nfx <= _lib.PQ_PG_WMB:
        return "wide"
    if k > 256 or ma > RT_WMA:
        return "per-date fallback"
    return SOLVERS[0 if k <= 48 else 1 if k <= 64 else 2 if k <= 80 else 3 if k <= 96 else 4 if k <= 128 else 5]


def _observed(nfree, state, wide):
    if state == _lib.PQ_PG_FALLBACK:
        return "per-date fallback"
    return "wide" if wide else _expected("", int(nfree), 0, 0)


@functools.lru_cache(maxsize=None)
def _problem(device, fam):
    """The family's batch on the device, its optima manufactured with the device's own window means."""
    bw = mf.family_windows(fam)
    n, D = bw.n, bw.D
    pan = engine.Panel(bw.R, device=device)
    r_d, t_d = pan.rows_to_device(bw.rows, bw.tlen)
    mu = pan.window_means(r_d, t_d) if bw.centred else None
    b = mf.family(fam, mu=None if mu is None else mu[:, :n].cpu().numpy().copy())
    G = b.C[1:] if b.C.shape[0] > 1 else None
    qb = engine.QPBatch.from_dense(None, None, A=b.C[:1], b=b.ug[:1], G=G, h=None if G is None else b.ug[1:],
                                   lb=b.lb, ub=b.ub, device=device, n=n)
    qb.batch = D
    qb.p_scale = torch.full((D,), b.p_scale, dtype=F64, device=device)
    qb.p_diag = torch.tensor([o.p_diag for o in b.opt], dtype=F64, device=device)
    q = np.zeros((D, qb.ld))
    q[:, :n] = np.stack([o.q for o in b.opt])
    qb.q = torch.from_numpy(q).to(device)
    lr = engine.LowRank(pan, r_d, t_d, mu=mu, w_scale=1.0 / (t_d.to(F64) - 1.0) if bw.centred else None)
    gp = engine.GroupPlan(b.rows, b.tlen, device, cus=1, breaks=b.breaks)
    assert gp.ok
    if fam == "A":
        assert gp.sizes.tolist() == [14, 2, 16, 16] and gp.gcap_plan().sizes.tolist() == [14, 10, 24]
    return b, pan, qb, lr, gp


def _settings(mode):
    st = engine.Settings()
    if mode == "default":
        return st
    return dataclasses.replace(st, **TIGHT, refine_iters=st.refine_retry if mode == "tight-retry" else st.refine_iters)


@functools.lru_cache(maxsize=None)
def _run(device, fam, mode, polish=True):
    """One solve; host copies of the answer, the record and the certificate."""
    b, pan, qb, lr, gp = _problem(device, fam)
    st = _settings(mode)
    ws = engine.Workspace(qb, dense=False)
    assert ws.ldk == 256 and engine.grouped_applicable(qb, lr, gp, ws)
    res = engine.solve_lowrank(qb, lr, st, ws=ws, groups=gp, polish=polish)
    torch.cuda.synchronize()
    assert res.capacitance == "group" and ws.gcap_groups is not None   # every group has one p_diag
    n, mg = qb.n, qb.mg
    out = dict(x=res.x.cpu().numpy().copy(), y=res.y.cpu().numpy().copy(), zb=res.z_box.cpu().numpy().copy(),
               status=res.status.cpu().numpy().copy(), out=res.out.cpu().numpy().copy(),
               iters=res.iters.cpu().numpy().copy(), fallbacks=res.polish_fallbacks)
    if polish:
        out["rec"] = ws.pg_record().cpu().numpy().copy()
        scale = qb.p_scale * (lr.w_scale if lr.w_scale is not None else 1.0)
        out["cert"] = window_certificate(pan.R, lr.rows, lr.tlen, lr.mu, scale, qb.q[:, :n], res, lb=qb.lb[0, :n],
                                         ub=qb.ub[0, :n], C=qb.Cg[0, :mg, :n], lg=qb.lg[0, :mg], ug=qb.ug[0, :mg],
                                         p_diag=qb.p_diag)
    return out


def _end_state(tag, b, r):
    """Bars (a) and (b) on the end state of every date."""
    n = b.n
    eq = b.lg == b.ug
    worst = dict(x=0.0, obj=0.0, viol=0.0)
    assert np.all(r["status"] == _lib.PQ_SOLVED), (tag, r["status"])
    for d, o in enumerate(b.opt):
        x, zb = r["x"][d], r["zb"][d]
        inside = np.flatnonzero((b.lb < x) & (x < b.ub))
        assert np.array_equal(inside, o.F), (tag, d, o.k, len(inside), np.setxor1d(inside, o.F))
        assert np.array_equal(np.flatnonzero(zb == 0.0), o.F), (tag, d, o.k)
        assert r["out"][d, _lib.PQ_OUT_NFREE] == o.k, (tag, d, o.k, r["out"][d, _lib.PQ_OUT_NFREE])
        P = mf.window_P(b.X(d), None if b.mu is None else b.mu[d], b.psw(d), o.p_diag)
        obj_ref = float(0.5 * o.x @ (P @ o.x) + o.q.astype(LD) @ o.x)
        cx = b.C @ x
        viol = max(np.abs(cx - b.ug)[eq].max(), np.maximum(cx - b.ug, 0.0).max(), np.maximum(b.lb - x, 0.0).max(),
                   np.maximum(x - b.ub, 0.0).max())
        e = dict(x=float(np.abs(x - o.x).max()), obj=abs(r["out"][d, _lib.PQ_OUT_OBJ] - obj_ref) / abs(obj_ref),
                 viol=float(viol))
        assert e["x"] <= 1e-5 and e["obj"] <= 1e-6 and e["viol"] <= 1e-7, (tag, d, o.k, e)
        worst = {k: max(worst[k], e[k]) for k in worst}
    c = r["cert"]
    print(f"[buckets] {tag}: worst |x - x*| {worst['x']:.1e}  obj {worst['obj']:.1e}  violation {worst['viol']:.1e}  "
          f"certificate viol {c['max_violation']:.1e} stat {c['max_rel_stationarity']:.1e} "
          f"comp {c['max_rel_complementarity']:.1e}; ADMM iterations {r['iters'].min()}..{r['iters'].max()}, rounds "
          f"{r['out'][:, _lib.PQ_OUT_ROUNDS].min():.0f}..{r['out'][:, _lib.PQ_OUT_ROUNDS].max():.0f}, "
          f"fallbacks {r['fallbacks']}")
    assert c["max_violation"] <= 1e-9, c
    assert c["max_rel_stationarity"] <= 1e-8 and c["max_rel_complementarity"] <= 1e-8 and c["max_dual_sign"] <= 1e-8, c


def _census(tag, fam, b, r):
    """Tight mode: the record says the solver k_d selects took the date's last round."""
    census = {}
    for d, o in enumerate(b.opt):
        rec = r["rec"][d]
        ma, nfx = int(o.act.sum()), b.n - o.k
        want = _expected(fam, o.k, ma, nfx)
        got = _observed(r["out"][d, _lib.PQ_OUT_NFREE], rec[_lib.PQ_PG_STATE], rec[_lib.PQ_PG_W] == 1.0)
        assert got == want, (tag, d, o.k, ma, nfx, got, want)
        assert rec[_lib.PQ_PG_W] == (1.0 if want == "wide" else 0.0), (tag, d, o.k)
        if want == "per-date fallback":
            assert rec[_lib.PQ_PG_STATE] == _lib.PQ_PG_FALLBACK, (tag, d, o.k)
        else:
            assert rec[_lib.PQ_PG_STATE] == _lib.PQ_PG_DONE and rec[_lib.PQ_PG_K] == o.k, (tag, d, o.k, rec[:8])
            if want != "wide":
                assert rec[R_KB] == o.k, (tag, d, o.k, rec[R_KB])
        census[want] = census.get(want, 0) + 1
    print(f"[buckets] {tag}: dates per solver {census}")
    return census


def _tight_bar(tag, fam, b, r, adm, st):
    """Bar (c), for the dates whose last round ran on a modelled solver."""
    missed = []
    for d, o in enumerate(b.opt):
        solver = _expected(fam, o.k, int(o.act.sum()), b.n - o.k)
        if solver not in MODELLED:
            continue
        X, mu = b.X(d), None if b.mu is None else b.mu[d]
        sc = mf.problem_scale(X, mu, b.psw(d), o.p_diag, o.q)
        assert abs(sc / r["rec"][d, _lib.PQ_PG_SC] - 1.0) <= 1e-12     # the kernels' own problem scale
        xm, lm, zm, steps = mf.reduced_kkt_f64(X, mu, b.psw(d), o.p_diag, o.q, b.C, b.lg, b.ug, b.lb, b.ub, o.side,
                                               o.act, adm["x"][d], adm["y"][d], st.delta * sc, st.refine_iters,
                                               stop=mf.STOP_REL * sc)
        xs = np.abs(o.x).max()
        dist = lambda x, lam, zb: (float(np.abs(x - o.x).max() / xs),
                                   float(max(np.abs(lam - o.lam).max(), np.abs(zb - o.z).max()) / o.s))
        dk, dm, d0 = dist(r["x"][d], r["y"][d], r["zb"][d]), dist(xm, lm, zm), dist(adm["x"][d], adm["y"][d], adm["zb"][d])
        print(f"[buckets] bar (c) {tag} date {d:2d} k {o.k:3d} {solver:12s} model steps {steps}  ADMM point {d0[0]:.1e} "
              f"{d0[1]:.1e}  x {dk[0]:.1e} / {dm[0]:.1e}  multipliers {dk[1]:.1e} / {dm[1]:.1e}")
        for what, k_, m_ in zip(("x", "multipliers"), dk, dm):
            s = RATIOS.setdefault((solver, what), [0.0, 0.0, 0.0])
            if k_ / m_ > s[0]:
                s[:] = [k_ / m_, k_, m_]
            assert 10.0 * m_ <= 1e-9, (tag, d, o.k, what, m_)              # the bar is never looser than 1e-9
            if not k_ <= 10.0 * m_ + 1e-14:
                missed.append((d, o.k, solver, what, k_, m_))
    for solver in MODELLED:
        for what in ("x", "multipliers"):
            if (solver, what) in RATIOS:
                s = RATIOS[(solver, what)]
                print(f"[buckets] bar (c) so far {solver:12s} {what:11s} worst d_kernel / d_model {s[0]:6.2f} "
                      f"({s[1]:.1e} / {s[2]:.1e})")
    assert not missed, (tag, missed)


@pytest.mark.parametrize("mode", ["tight", "tight-retry"])
@pytest.mark.parametrize("fam", mf.FAMILIES)
def test_tight_mode_last_round_runs_on_the_solver_k_selects(device, fam, mode):
    b = _problem(device, fam)[0]
    r = _run(device, fam, mode)
    tag = f"{fam} {mode}"
    _end_state(tag, b, r)
    census = _census(tag, fam, b, r)
    want = {}
    for o in b.opt:
        s = _expected(fam, o.k, int(o.act.sum()), b.n - o.k)
        want[s] = want.get(s, 0) + 1
    assert census == want and all(v >= 2 for v in census.values()), (census, want)
    if fam == "A":     # every solver but the wide rounds, from this one batch
        assert set(census) == set(SOLVERS) - {"wide"}, census
    if fam == "C8":    # 9 active rows: every date handed to the per-date kernel
        assert census == {"per-date fallback": b.D}, census
    if fam == "W":
        assert census == {"wide": 6, "per-date fallback": 2}, census
    if mode == "tight-retry":
        adm = _run(device, fam, mode, polish=False)
        assert np.all(adm["status"] == _lib.PQ_SOLVED), adm["status"]
        _tight_bar(tag, fam, b, r, adm, _settings(mode))


@pytest.mark.parametrize("fam", mf.FAMILIES)
def test_default_settings_end_on_the_manufactured_optimum(device, fam):
    """engine.Settings() as shipped: only the end state (dates may legitimately be handed to the repairs)."""
    b = _problem(device, fam)[0]
    _end_state(f"{fam} default", b, _run(device, fam, "default"))


def test_every_solver_is_reached(device):
    """Over the module's tight runs every solver solved at least two dates."""
    census = {}
    for fam in mf.FAMILIES:
        b = _problem(device, fam)[0]
        for mode in ("tight", "tight-retry"):
            r = _run(device, fam, mode)
            for d, o in enumerate(b.opt):
                rec = r["rec"][d]
                s = _observed(r["out"][d, _lib.PQ_OUT_NFREE], rec[_lib.PQ_PG_STATE], rec[_lib.PQ_PG_W] == 1.0)
                census[s] = census.get(s, 0) + 1
    print(f"[buckets] module census (both tight modes): {census}")
    for s in SOLVERS:
        assert census.get(s, 0) >= 2, (s, census)
