"""The iterates of every low-rank ADMM entry point against a dense extended-precision model of
the same iteration (tests/admm_reference.py: np.longdouble, K solved densely with iterative
refinement) -- not against another kernel:

    pq_admm_lr_batched                      'per-problem'
    pq_admm_lr_grouped, unfused and fused   'grouped-unfused', 'grouped-fused'
    pq_admm_lr_gcap, 16- and 32-date form   'gcap16', 'gcap32' (register-resident general rows;
                                            column-sparse wide form with 8 sector caps)
    pq_admm_lr_sweep, M^-1 from the         'sweep-chol', 'sweep-eig'
    Cholesky and from the eigen form

Every case first asserts which kernel ran.  Then, through engine.solve_lowrank /
MeanVarianceSweep with polish = 0, eps 1e-12, no loose stop and no adaptation, the state after
ITERS iterations (x, z and y over the rows [general; box], Px) is read back together with the
kernel's own inputs (panel rows, window means, p_scale w_scale, q, rows, boxes, ws.rho) and

    d_kernel = max_b |kernel - ref|_inf / |ref|_inf  <=  10 d_model + 1e-14

where d_model is the same distance for the float64 numpy model of the kernels' algebra
(admm_woodbury_f64: K^-1 = (I - V'M^-1 V / d) / d with an explicit inv(M)).  The kernels
differ from that model only in summation order and fma contraction; 10 is the project's
margin between summation orders (tests/test_sweep_admm_gpu.py).

ITERS = 7 (the headline benchmark's ADMM runs exactly 7 iterations).  The bar is meant to stay
under 1e-6 (10 d_model <= 1e-6 by the reference alone), and the iteration count is the lever:
at 9 iterations y, whose scale shrinks as the iteration converges, misses it on the first
sweep shape (d_model 1.2e-7, CPU); at 7 it holds for z and y on every shape (d_model <= 3.9e-8)
and for x on every sweep shape and three of the five sliding cases (<= 7.3e-8).  Where it does NOT
hold, by the reference alone and at any iteration count from 2 on:
  * x, uncentred 282 x 150 windows: d_model 1.9e-7 (2.0e-7 .. 2.6e-7 at 3 .. 9 iterations on the
    CPU; the market mode stays in X'X and the budget row's 1e3 rho cancels ~5 digits in
    rhs - V'u), and x with the 8 sector caps: 1.4e-7 (2.2e-7 at the 16-date groups' rho);
  * Px, every shape with a budget row: d_model 1.5e-5 .. 1.0e-2.  Px~ = rhs - sigma x~ - C'(rv z~)
    is the residual of the K solve: the explicit-inverse Woodbury solve leaves ~2e-9 |rhs|, and
    |rhs| carries the budget row's rho eq_scale (~1e2) against |Px| of 1e-5 .. 1e-2.  The
    kernels' Px, and with it their dual residual, is good to ~1e-7 absolute and no better.
So besides the 10 d_model bar (all four vectors) the test asserts d_kernel <= 1e-6 outright
for x, z and y: the bar is never looser than it was designed to be.  Px keeps the 10 d_model
bar alone.

Shapes, and the tile constant each was chosen against:
  n = 282  admm_sweep.hip SW_CH = 256 / SW_SA = 16: a second chunk of one full 16-asset
           sub-chunk and a ragged 10; 32-lane half-wave strides of admm_grp / admm_gcap
           (8 x 32 + 26); n = 300: 9 x 32 + 12
  T = 150  admm_sweep.hip's two 128-row K halves (SW_K = 256), not a multiple of 16;
  T = 20   second K half all padding;  L = 70: groups of 64 + 6 (SW_G = 64), L = 40: one group
  D = 40   admm_grp GMAX = 16: groups 16 + 16 + 8 (stride 1) and 14 + 14 + 12 (stride 3);
           admm_gcap CG_MAX = 16 x NB = 2: 32 + 8 (stride 1) and 20 + 20 (stride 3: the
           correction rank 3 (G - 1) + 1 <= CH_MAX = 64 caps a group at 22 dates), i.e. a
           ragged second column block either way
  unions   U = 93 .. 117 (stride 3) and 157 .. 181 rows (stride 1): ragged 16-row MFMA tiles,
           below CU_MAX = 320

Measured on an MI355X, worst over the cases: d_kernel <= ... / d_model (worst d_kernel / d_model)
  sweep batch, mg = 1 and 3     x                z                y                Px
    per-problem                 1.3e-9 / 2.9e-9  8.8e-10 / 2.4e-10  1.8e-8 / 1.5e-8  7.2e-3 / 2.4e-3  (0.9)
    grouped-fused               9.9e-10          1.0e-9             2.3e-8           6.1e-3           (1.1)
    sweep-chol                  1.3e-9           1.1e-9             1.8e-8           1.0e-2           (1.1)
    sweep-eig                   1.1e-9           9.7e-10            2.4e-8           1.1e-2           (1.1)
  sweep batch, mg = 0 (box only): every form and vector 6e-15 .. 4.8e-14 / 3.7e-15 .. 4.4e-14 (2.7)
  sliding batch                 x                z                y                Px
    per-problem                 7.1e-9 / 4.7e-8  5.7e-10 / 8.1e-10  3.4e-8 / 1.3e-8  1.2e-4 / 1.5e-5  (1.6)
    grouped-unfused             6.4e-9           5.6e-10            3.4e-8           1.2e-4           (1.6)
    grouped-fused               8.2e-9           5.5e-10            3.2e-8           1.2e-4           (1.6)
    gcap16                      9.8e-9 / 3.3e-8  5.9e-10 / 5.7e-10  5.1e-8 / 1.2e-8  2.7e-4 / 1.7e-5  (3.8)
    gcap32                      1.3e-8 / 2.6e-8  8.8e-10 / 3.4e-10  7.6e-8 / 1.4e-8  3.3e-4 / 2.1e-5  (4.8)
  (d_model: the smallest over the cases; it is the same for the forms that share a rho -- the
  group capacitance runs every group at the mean of its dates' rho.)  The worst ratios are the
  32-date form's Px (4.8, with the sector caps) and y (4.0, centred 282 x 150): within the 10.
  adaptive rho: |rho / rho_ref - 1| 7.5e-9 .. 1.3e-8 against the model's 5.1e-8; 80 refactorisations.

Stop rule: with eps 1.6e-3, min_iter 3, max_iter 60 every iteration count and status equals
the reference's on all four sweep forms; by the reference alone every rp / eps_p and
rd / eps_d of every iteration is >= 1e-3 away from 1 (at 2e-3 one problem sat
7e-5 from the edge; 1.6e-3 leaves 1.8e-3; 26 .. 43 iterations).  Adaptive rho (interval 4,
tol 1.5, max_iter 12): refactorisations happen, counts equal the reference's, rho within 10x
the float64 model's own rho distance.  Every problem of that batch asks for a new rho at
iterations 8 and 12: the request at max_iter itself once left the grouped and the sweep
kernel one iteration beyond max_iter (13) and the per-problem kernel with a rho no
iteration used; no entry point asks at max_iter any more.
"""
import dataclasses

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.sweep import SWEEP_SETTINGS, MeanVarianceSweep
from porqua_amd.synthetic import factor_panel
from tests.admm_reference import LD, admm_dense_ref, admm_woodbury_f64, rel_dist
from tests.test_gcap_gpu import _problem

pytestmark = pytest.mark.gpu

ITERS = 7
VECS = ("x", "z", "y", "Px")
STATUS = {"solved": _lib.PQ_SOLVED, "max_iter": _lib.PQ_MAX_ITER, "unsolved": _lib.PQ_UNSOLVED}
FIXED = dict(polish=0, eps_abs=1e-12, eps_rel=1e-12, eps_grouped=0.0, adapt_interval=0)


# ---- the kernel's inputs and state, read back from the device --------------------------------

def _inputs(qb, lr, ws):
    """The kernels' own inputs, read back.  Shared rows and a box whose rows all take one rho (the two
    asserts): what they exclude -- fixed variables and one-sided rows among ordinary ones, per-problem
    rows and boxes, i.e. the direct capacitance with the per-problem and the unfused grouped ADMM -- is
    covered by tests/test_window_mixed_gpu.py."""
    n, mg, B = qb.n, qb.mg, qb.batch
    one = torch.ones(B, dtype=torch.float64, device=qb.device)
    assert qb.shared and qb.lb.shape[0] == 1
    ps = (qb.p_scale if qb.p_scale is not None else one) * (lr.w_scale if lr.w_scale is not None else one)
    lb, ub = qb.lb[0, :n].cpu().numpy(), qb.ub[0, :n].cpu().numpy()
    assert np.all(lb < ub)   # (the kernels classify the box rows by asset 0 alone)
    return dict(n=n, mg=mg, B=B, R=lr.panel.R[:, :n].cpu().numpy(), rows=lr.rows.cpu().numpy(),
                tlen=lr.tlen.cpu().numpy(), mu=None if lr.mu is None else lr.mu[:, :n].cpu().numpy(),
                ps=ps.cpu().numpy(), pd=None if qb.p_diag is None else qb.p_diag.cpu().numpy(),
                q=qb.q[:, :n].cpu().numpy(), Cg=qb.Cg[0, :mg, :n].cpu().numpy(),
                lg=qb.lg[0, :mg].cpu().numpy(), ug=qb.ug[0, :mg].cpu().numpy(), lb=lb, ub=ub,
                rho=ws.rho.cpu().numpy().copy())


def _state(qb, ws):
    n, mg, p = qb.n, qb.mg, ws.mg_pad
    torch.cuda.synchronize()
    z, y = ws.z.cpu().numpy(), ws.y.cpu().numpy()
    return dict(x=ws.x[:, :n].cpu().numpy().copy(), Px=ws.Px[:, :n].cpu().numpy().copy(),
                z=np.concatenate([z[:, :mg], z[:, p:p + n]], 1), y=np.concatenate([y[:, :mg], y[:, p:p + n]], 1),
                iters=ws.iters.cpu().numpy().copy(), status=ws.status.cpu().numpy().copy(),
                rho=ws.rho.cpu().numpy().copy())


class _Reference:
    """The dense model (and the float64 yardstick) of one batch: the window Grams are formed
    once per distinct window in longdouble and shared by its problems; a run is cached per
    (rho, settings), so the forms of a case that use the same rho share it."""

    def __init__(self):
        self.grams, self.runs = {}, {}

    def _window(self, inp, b):
        rows = inp["rows"][b, :inp["tlen"][b]]
        key = (rows.tobytes(), None if inp["mu"] is None else inp["mu"][b].tobytes())
        if key not in self.grams:
            X = inp["R"][rows]
            Xc = X if inp["mu"] is None else X - inp["mu"][b]
            Xl = X.astype(LD) if inp["mu"] is None else X.astype(LD) - inp["mu"][b].astype(LD)
            self.grams[key] = (Xc, Xl.T @ Xl)
        return self.grams[key]

    def run(self, inp, st, iters, rho=None, model=True):
        rho = inp["rho"] if rho is None else rho
        key = (rho.tobytes(), inp["q"].tobytes(), repr(dataclasses.astuple(st)), iters, model)
        if key in self.runs:
            return self.runs[key]
        assert inp["pd"] is None
        ref, mod = [], []
        for b in range(inp["B"]):
            Xc, S = self._window(inp, b)
            a = (inp["q"][b], inp["Cg"], inp["lg"], inp["ug"], inp["lb"], inp["ub"], rho[b], st, iters)
            ref.append(admm_dense_ref(LD(inp["ps"][b]) * S, *a))
            if model:
                mod.append(admm_woodbury_f64(Xc, inp["ps"][b], *a))
        self.runs[key] = (ref, mod)
        return ref, mod


def _dist(rows, ref, k):
    """max over the problems of |a_b - ref_b|_inf / |ref_b|_inf."""
    return max(rel_dist(rows[b], getattr(ref[b], k)) for b in range(len(ref)))


def _compare(tag, state, ref, mod):
    """The bar of the module docstring for x, z, y, Px; returns {vector: (d_kernel, d_model)}."""
    out = {k: (_dist(state[k], ref, k), _dist([getattr(m, k) for m in mod], ref, k)) for k in VECS}
    print("ITERATES %-34s " % tag + "  ".join("%s %.1e/%.1e" % (k, *out[k]) for k in VECS))
    assert np.all(state["iters"] == ITERS) and np.all(state["status"] == _lib.PQ_MAX_ITER)
    assert all(r.iters == ITERS and r.status == "max_iter" for r in ref)
    for k in VECS:
        dk, dm = out[k]
        assert dk <= 10.0 * dm + 1e-14, (tag, k, dk, dm)
        if k != "Px":   # never looser than the 1e-6 the bar was designed to stay under (docstring)
            assert dk <= 1e-6, (tag, k, dk)
    return out


# ---- the sweep batch: P = 2 lam Sigma_d, q = -mu_d, 2 dates at stride 21 ---------------------

SWEEP_FORMS = ("per-problem", "grouped-fused", "sweep-chol", "sweep-eig")
SWEEP_CASES = {   # n, T, L, mg, ub
    "n282-T150-L70-mg1": (282, 150, 70, 1, 1.0),
    "n282-T20-L40-mg3": (282, 20, 40, 3, 1.0),
    "n282-T20-L40-mg0": (282, 20, 40, 0, 0.05),
    "n282-T20-L40-mg1": (282, 20, 40, 1, 1.0),    # (the stop-rule and adaptive-rho batch)
}
_refs = {}


def _general_rows(sw, mg):
    """mg = 3: the budget, a cap on the first third (<= 0.3) and a floor on the second
    (>= 0.1), one-sided rows; mg = 0: box only.  (mg = 1: the sweep's own budget row.)"""
    if mg == 1:
        return
    n, dev = sw.n, sw.device
    qb = engine.QPBatch(n, sw.B, mg, device=dev, P=torch.empty(0, dtype=torch.float64, device=dev))
    qb.P = None
    qb.lb, qb.ub, qb.p_scale = sw.qb.lb, sw.qb.ub, sw.qb.p_scale
    if mg == 3:
        qb.Cg[0, 0, :n] = 1.0
        qb.Cg[0, 1, :n // 3] = 1.0
        qb.Cg[0, 2, n // 3:2 * (n // 3)] = 1.0
        qb.lg[0, :] = torch.tensor([1.0, -np.inf, 0.1], dtype=torch.float64)
        qb.ug[0, :] = torch.tensor([1.0, 0.3, np.inf], dtype=torch.float64)
    else:
        assert mg == 0
    sw.qb = qb
    sw.ws = engine.Workspace(qb, dense=False)


def _run_sweep(device, case, form, settings):
    n, T, L, mg, ub = SWEEP_CASES[case]
    stride, dates = 21, 2
    d_all, R, _, _ = factor_panel(T - 1 + stride * dates, n)
    ends = np.arange(T - 1, T - 1 + stride * dates, stride)
    rows, tlen = engine.window_rows(d_all, d_all[ends], T)
    assert np.all(tlen == T)   # full windows (the eigen form needs them)
    pan = engine.Panel(R, device=device)
    st = engine.Settings.from_params({**SWEEP_SETTINGS, **settings})
    sw = MeanVarianceSweep(pan, rows, tlen, np.logspace(-1, 2, L), ub=ub, settings=st,
                           factor="eig" if form == "sweep-eig" else "chol")
    _general_rows(sw, mg)
    if form == "grouped-fused":
        sw.sp = None
    elif form == "per-problem":
        sw.sp = sw.gp = None
    res, meta = sw.solve()
    torch.cuda.synchronize()
    # which kernel ran
    ws = sw.ws
    assert res.capacitance == ("eig" if form == "sweep-eig" else "band") and ws.gcap_groups is None
    if form.startswith("sweep"):
        assert sw.sp is not None and ws.sweep_admm is sw.sp and sw.sp.ngroups == dates * ((L + 63) // 64)
        assert meta["factor"] == ("eig" if form == "sweep-eig" else "chol")
    else:
        assert getattr(ws, "sweep_admm", None) is None
        assert (form == "grouped-fused") == (sw.gp is not None and engine.grouped_applicable(sw.qb, sw.lr, sw.gp, ws))
    return sw, res, st


@pytest.mark.parametrize("form", SWEEP_FORMS)
@pytest.mark.parametrize("case", list(SWEEP_CASES)[:3])
def test_sweep_batch_iterates(device, case, form):
    sw, res, st = _run_sweep(device, case, form, {**FIXED, "max_iter": ITERS})
    inp, state = _inputs(sw.qb, sw.lr, sw.ws), _state(sw.qb, sw.ws)
    assert res.refactors == 0
    ref, mod = _refs.setdefault(case, _Reference()).run(inp, st, ITERS)
    _compare(f"{case} {form}", state, ref, mod)


# ---- the sliding-window batch: min variance / tracking, tests/test_gcap_gpu.py::_problem -----

SLIDE_FORMS = ("per-problem", "grouped-unfused", "grouped-fused", "gcap16", "gcap32")
# n, T, D, ub, stride, centred, caps, gmin.  The plans are built for one CU (cus = 1), so that 40
# dates make full groups: gmin = 32 gives 16 + 16 + 8 dates and the 32-date plan 32 + 8; the
# plan's own balancing (gmin = 4) gives 14 + 14 + 12 and 20 + 20 -- the stride-3 windows need
# it: their Woodbury correction has rank 3 (G - 1) + 1 <= 64 (admm_gcap.hip CH_MAX), G <= 22
SLIDE_CASES = {
    "n300-T60-s3-centred": (300, 60, 40, 0.2, 3, True, 0, 4),
    "n300-T60-s3-uncentred": (300, 60, 40, 0.2, 3, False, 0, 4),
    "n282-T150-s1-centred": (282, 150, 40, 1.0, 1, True, 0, 32),
    "n282-T150-s1-uncentred": (282, 150, 40, 1.0, 1, False, 0, 32),
    "n300-T60-s3-centred-caps8": (300, 60, 40, 0.2, 3, True, 8, 4),
}


def _run_slide(device, case, form):
    n, T, D, ub, stride, centred, caps, gmin = SLIDE_CASES[case]
    qb, lr, gp = _problem(device, n, T, D, ub, stride, centred=centred, caps=caps)
    gp = engine.GroupPlan(*gp._host[:2], device, cus=1, gmin=gmin)
    assert gp.ok and gp.sizes.tolist() == ([16, 16, 8] if gmin == 32 else [14, 14, 12])
    st = engine.Settings(**{**FIXED, "max_iter": ITERS})
    ws = engine.Workspace(qb, dense=False)
    gcap = form.startswith("gcap")
    old = engine.GCAP_MAX_DATES
    try:
        if form == "gcap16":
            engine.GCAP_MAX_DATES = 16
        res = engine.solve_lowrank(qb, lr, st, ws=ws, polish=False, groups=None if form == "per-problem" else gp,
                                   gcap=gcap, fuse=form != "grouped-unfused")
    finally:
        engine.GCAP_MAX_DATES = old
    torch.cuda.synchronize()
    # which kernel ran
    assert getattr(ws, "sweep_admm", None) is None
    if gcap:
        assert res.capacitance == "group"
        if form == "gcap16":
            assert ws.gcap_groups is gp
        else:
            g32 = gp.gcap_plan()
            assert ws.gcap_groups is g32 and g32 is not gp
            assert g32.sizes.tolist() == ([32, 8] if gmin == 32 else [20, 20])
    else:
        assert res.capacitance == "band" and ws.gcap_groups is None
        assert form == "per-problem" or engine.grouped_applicable(qb, lr, gp, ws)
    assert (qb.mg > 4) == (caps > 0) and (engine._sparse_columns(qb)[2] > 0) == (caps > 0)
    return qb, lr, ws, res, st


@pytest.mark.parametrize("form", SLIDE_FORMS)
@pytest.mark.parametrize("case", list(SLIDE_CASES))
def test_sliding_batch_iterates(device, case, form):
    qb, lr, ws, res, st = _run_slide(device, case, form)
    inp, state = _inputs(qb, lr, ws), _state(qb, ws)
    assert res.refactors == 0
    ref, mod = _refs.setdefault(case, _Reference()).run(inp, st, ITERS)
    _compare(f"{case} {form}", state, ref, mod)


# ---- stop rule and adaptive rho on the four sweep forms --------------------------------------

STOP_CASE = "n282-T20-L40-mg1"
STOP = dict(polish=0, eps_abs=1.6e-3, eps_rel=1.6e-3, eps_grouped=0.0, adapt_interval=0, min_iter=3, max_iter=60)
ADAPT = {**FIXED, "adapt_interval": 4, "adapt_tol": 1.5, "max_iter": 12}


def _initial_rho(device):
    """The initial rho of the batch (ws.rho after a run without adaptation)."""
    if "rho0" not in _refs:
        sw, _, _ = _run_sweep(device, STOP_CASE, "per-problem", {**FIXED, "max_iter": 1})
        _refs["rho0"] = sw.ws.rho.cpu().numpy().copy()
    return _refs["rho0"]


@pytest.mark.parametrize("form", SWEEP_FORMS)
def test_sweep_batch_stop_rule_counts(device, form):
    sw, res, st = _run_sweep(device, STOP_CASE, form, STOP)
    inp, state = _inputs(sw.qb, sw.lr, sw.ws), _state(sw.qb, sw.ws)
    assert np.array_equal(inp["rho"], _initial_rho(device))
    ref, _ = _refs.setdefault(STOP_CASE, _Reference()).run(inp, st, st.max_iter, model=False)
    # by the reference alone: no stop decision rests on rounding
    edge = min(min(abs(rp / ep - 1.0), abs(rd / ed - 1.0)) for r in ref for rp, ep, rd, ed in r.hist)
    it_ref = np.array([r.iters for r in ref])
    print("STOP %s: reference iterations %d..%d, nearest residual/eps to 1: %.2e"
          % (form, it_ref.min(), it_ref.max(), edge))
    assert edge >= 1e-3, edge
    assert it_ref.min() >= st.min_iter and len(np.unique(it_ref)) > 4 and it_ref.max() < st.max_iter
    assert np.array_equal(state["iters"], it_ref), (state["iters"], it_ref)
    assert np.array_equal(state["status"], np.array([STATUS[r.status] for r in ref]))


@pytest.mark.parametrize("form", SWEEP_FORMS)
def test_sweep_batch_adaptive_rho(device, form):
    rho0 = _initial_rho(device)
    sw, res, st = _run_sweep(device, STOP_CASE, form, ADAPT)
    inp, state = _inputs(sw.qb, sw.lr, sw.ws), _state(sw.qb, sw.ws)
    ref, mod = _refs.setdefault(STOP_CASE, _Reference()).run(inp, st, st.max_iter, rho=rho0)
    assert res.refactors > 0
    rho_ref = np.array([r.rho for r in ref])
    assert np.any(rho_ref != rho0)
    assert np.array_equal(state["iters"], np.array([r.iters for r in ref])), state["iters"]
    assert np.array_equal(state["status"], np.array([STATUS[r.status] for r in ref])), state["status"]
    d_model = np.abs(np.array([m.rho for m in mod]) / rho_ref - 1.0).max()
    d_kernel = np.abs(state["rho"] / rho_ref - 1.0).max()
    print("ADAPT %s: rho d_kernel %.1e d_model %.1e refactors %d" % (form, d_kernel, d_model, res.refactors))
    assert d_kernel <= 10.0 * d_model, (d_kernel, d_model)
