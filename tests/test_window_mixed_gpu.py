"""The window-form solve on the route tests/test_admm_iterates_gpu.py excludes by its asserts: box
rows that do not share one ADMM rho (fixed variables, one-sided rows) and per-problem
constraints.  engine._band_applies is false there, so solve_lowrank builds the capacitance
"direct" (pq_lr_capacitance / k_lr_gram with a per-asset D_c = sigma + p_diag + row_rho(lb_c, ub_c))
and the ADMM runs as pq_admm_lr_batched ('per-problem') or as the unfused pq_admm_lr_grouped
('grouped-unfused'), both reading lo_h[i] / up_h[i] per asset through box_stride, g_stride and
Cg_stride.  The inputs are tests/window_cases.py (split / mixed / perproblem boxes), built from
host arrays; every test first checks that the device holds exactly those arrays.

1. test_direct_capacitance_matches_longdouble: the lower triangle of every M_b against
   admm_reference.capacitance_ref (np.longdouble, U as lowrank.hip's header defines it),
   entry by entry:   |M_ij - ref_ij| <= N u S_ij,  S_ij = sum_c |U_ic U_jc| / D_c (+ 1 on the
   diagonal), u = 2^-53, N = 2 (n + 16) = 596: the gamma_n bound of the length-n contraction,
   doubled for the scalings sqrt(ps), sqrt(rho_r), 1 / sqrt(D_c) and their products (the
   convention of tests/residual_model.py).  S_ij <= max|M_b| (Cauchy-Schwarz), so this is never
   looser than N u max|M_b|.  General rows of every kind (equality, one-sided, two-sided,
   unbounded), ragged tlen, the idx argument (dates not asked for stay untouched).  Shapes: n = 282
   (no multiple of the 16-column chunk), T = 150, mg = 3: k = 153, k_ld = 192, three 64-row tile
   rows with a ragged last tile; T = 20, mg = 1: one tile, mostly padding.
   Observed on an MI355X, worst entry of each of the seven cases: 6.4 .. 11.3 u S_ij, i.e. 2.7 .. 9.6
   u max|M_b| (the float64 numpy form of the same product: 1.9 .. 9.6 u max|M_b|), against N = 596.

2. test_direct_route_iterates: tests/test_admm_iterates_gpu.py's method (polish = 0, eps 1e-12, no
   adaptation, ITERS = 7; x, z, y, Px read back) with d_model from admm_woodbury_diag_f64, the
   float64 numpy model of the per-asset-D algebra:
       d_kernel <= 10 d_model + 1e-14  (x, z, y, Px)   and   d_kernel <= 1e-6  (x, z, y).
   By the reference alone (tests/test_admm_reference.py) 10 d_model <= 1e-6 for x, z, y on every
   case and no d_model is below 1e-13, so the 1e-14 floor decides nothing.  Both forms are first
   asserted: lowrank_route says ("direct", form, no band), the result says "direct", no group
   capacitance, no sweep, no band Gram.  12 dates on one CU's plan: one group of 12, ragged against
   admm_grp.hip's GMAX = 16, at stride 1 (unions of T + 11 rows) and 3 (T + 33).
   Observed on an MI355X, worst d_kernel / smallest .. largest d_model (worst d_kernel / d_model):
     box, form                   x                           z                           y                           Px
     split       per-problem     8.6e-11 / 2.9e-11..1.1e-10 (1.1)  2.2e-10 / 5.0e-12..3.0e-10 (1.2)  1.0e-9 / 4.2e-10..9.4e-10 (2.0)  2.2e-8 / 3.8e-9..2.2e-8 (2.2)
     split       grouped-unfused 8.9e-11 (1.1)               2.5e-10 (1.3)               9.0e-10 (1.3)               1.8e-8 (1.6)
     mixed       per-problem     8.4e-10 / 2.5e-11..5.2e-9 (1.4)   7.5e-10 / 7.2e-12..2.1e-9 (0.9)   1.7e-9 / 3.9e-10..1.3e-9 (2.3)   1.1e-7 / 1.7e-8..9.6e-8 (2.4)
     mixed       grouped-unfused 8.8e-10 (1.3)               7.3e-10 (0.8)               1.4e-9 (2.3)                1.2e-7 (1.8)
     perproblem  per-problem     4.4e-10 / 1.9e-11..2.5e-9 (1.3)   6.2e-10 / 1.4e-11..1.6e-9 (1.3)   1.4e-9 / 3.5e-10..1.4e-9 (1.3)   8.2e-8 / 2.1e-8..8.5e-8 (1.4)
     perproblem  grouped-unfused 5.1e-10 (1.2)               5.0e-10 (1.1)               1.3e-9 (1.9)                7.5e-8 (1.8)

3. test_direct_route_stop_rule_counts / _adaptive_rho (282 x 20 centred, per-problem rows, mg = 3):
   iteration counts and statuses equal the longdouble reference's with eps 1.6e-3, min_iter 3
   (40 .. 50 iterations; by the reference alone no residual / eps ratio is within 1.18e-2 of 1);
   with interval 4, tol 1.5, max_iter 12 the refactorisation count equals the reference's accepted
   changes (12), the counts and statuses are equal and rho is within 10x the model's own rho
   distance (observed 2.7e-9 per-problem, 2.3e-9 grouped against the model's 2.2e-9).

4. test_free_rows_and_boxless_batches_are_certified: see its docstring.

Two deliberate breaks, each tried on a scratch build, fail here and in no earlier test: reading
lb[0], ub[0] for every asset in k_lr_gram's weights fails all of 1, 2, 3 and the free-row cases of
4 (and the direct-route cases of tests/test_out_record_gpu.py and tests/test_l1.py); dropping
hb * box_stride from the box rho in admm_grp.hip's next_rhs fails the twelve perproblem
grouped-unfused cases of 2 and the grouped-unfused cases of 3.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from tests import window_cases as wc
from tests.admm_reference import LD, capacitance_ref, rel_dist, row_rho
from tests.dense_cases import stop_edge

pytestmark = pytest.mark.gpu

ITERS = 7
VECS = ("x", "z", "y", "Px")
U64 = 2.0 ** -53
STATUS = {"solved": _lib.PQ_SOLVED, "max_iter": _lib.PQ_MAX_ITER, "unsolved": _lib.PQ_UNSOLVED}
FIXED = dict(polish=0, eps_abs=1e-12, eps_rel=1e-12, eps_grouped=0.0, adapt_interval=0)
FORMS = ("per-problem", "grouped-unfused")


def _check_inputs(case, qb, lr):
    """The device holds the case's host arrays, bit for bit, in the layout the kernels index."""
    n, mg, B, nc = case["n"], qb.mg, case["B"], case["nc"]
    h = lambda t: t.detach().cpu().numpy()
    assert qb.batch == B and qb.shared == (nc == 1) and qb.P is None
    c = qb.c_struct()
    assert (c.box_stride != 0) == (nc > 1 and case["lb"] is not None)
    assert (c.g_stride != 0) == (nc > 1) and (c.Cg_stride != 0) == (nc > 1)
    assert np.array_equal(h(qb.q[:, :n]), case["q"]) and np.array_equal(h(qb.Cg[:, :mg, :n]), case["Cg"])
    assert np.array_equal(h(qb.lg[:, :mg]), case["lg"]) and np.array_equal(h(qb.ug[:, :mg]), case["ug"])
    if case["lb"] is not None:
        assert np.array_equal(h(qb.lb[:, :n]), case["lb"]) and np.array_equal(h(qb.ub[:, :n]), case["ub"])
    assert np.array_equal(h(lr.panel.R), case["R"]) and np.array_equal(h(lr.rows), case["rows"])
    assert np.array_equal(h(lr.tlen), case["tlen"])
    if case["mu"] is not None:
        assert np.array_equal(h(lr.mu[:, :n]), case["mu"])
    ps = h(qb.p_scale) * (h(lr.w_scale) if lr.w_scale is not None else 1.0)
    assert np.array_equal(ps, case["ps"])
    assert (qb.p_diag is None) == (case["pd"] is None) and (qb.p_diag is None or np.array_equal(h(qb.p_diag), case["pd"]))


# ---- 1. the direct capacitance ---------------------------------------------------------------

CAP_CASES = {   # kind, n, T, mg, first row kind, ragged, idx
    "mixed-T150-mg3": ("mixed", 282, 150, 3, 0, False, None),          # equality, one-sided, two-sided
    "mixed-T150-mg3-ragged": ("mixed", 282, 150, 3, 1, True, None),    # one-sided, two-sided, unbounded
    "mixed-T20-mg1": ("mixed", 282, 20, 1, 3, False, None),            # unbounded: one tile, mostly padding
    "mixed-T150-mg3-idx": ("mixed", 282, 150, 3, 0, False, (3, 0)),
    "perproblem-T150-mg3": ("perproblem", 282, 150, 3, 0, False, None),   # (kinds rotate with the date)
    "perproblem-T150-mg3-ragged-idx": ("perproblem", 282, 150, 3, 2, True, (4, 1, 3)),
    "perproblem-T20-mg1": ("perproblem", 282, 20, 1, 0, False, None),
}


@pytest.mark.parametrize("name", list(CAP_CASES))
def test_direct_capacitance_matches_longdouble(device, name):
    kind, n, T, mg, first, ragged, idx = CAP_CASES[name]
    B = 5
    case = wc.window_case(kind, n, T, B, 2, centred=not ragged, mg=3 if mg == 3 else 1, pdiag=True, ragged=ragged)
    case["Cg"], case["lg"], case["ug"] = wc.kind_rows(n, case["nc"], mg, seed=5, first=first)
    qb, lr, _ = wc.to_device(case, device)
    _check_inputs(case, qb, lr)
    assert not engine._band_applies(qb, lr)
    kinds = {(bool(np.isfinite(l)), bool(np.isfinite(u)), bool(l == u)) for l, u in zip(case["lg"].ravel(), case["ug"].ravel())}
    assert len(kinds) == (4 if kind == "perproblem" else min(mg, 3))
    if ragged:
        assert case["tlen"].min() < T and case["tlen"].max() == T
    st = engine.Settings()
    ws = engine.Workspace(qb, dense=False)
    lib = _lib.load()
    L_, P_, S_ = ctypes.byref(lr.c_struct()), ctypes.byref(qb.c_struct()), ctypes.byref(ws.c_struct())
    SS, strm = ctypes.byref(st.to_c()), engine._stream()
    _lib.check(lib.pq_init_state_lr(L_, P_, S_, None, 0, SS, strm), "init")
    engine._rho_floor_q(qb, ws, st)
    k, k_ld = T + mg, engine.round_up(T + mg, 64)
    assert k_ld == (192 if T == 150 else 64)
    M = torch.zeros((B, k_ld, k_ld), dtype=torch.float64, device=device)
    it = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=device)
    _lib.check(lib.pq_lr_capacitance(L_, P_, S_, engine._ptr(it), 0 if idx is None else len(idx), SS, M.data_ptr(),
                                     k_ld, k_ld * k_ld, strm), "pq_lr_capacitance")
    torch.cuda.synchronize()
    Mh, rho = M.cpu().numpy(), ws.rho.cpu().numpy()
    rho_host = wc.initial_rho(case, st)
    assert np.abs(rho / rho_host - 1.0).max() <= 1e-12, (rho, rho_host)   # (the host formula the CPU tests use)
    N = 2 * (n + 16)
    low = np.tril(np.ones((k_ld, k_ld), dtype=bool))
    worst_s = worst_m = worst_model = 0.0
    for b in range(B):
        if idx is not None and b not in idx:
            assert not Mh[b].any()   # not asked for: untouched
            continue
        q, Cg, lg, ug, lb, ub = wc.problem_args(case, b)
        a = (wc.window_X(case, b), case["ps"][b], Cg, lg, ug, lb, ub, rho[b], st)
        ref = np.eye(k_ld, dtype=LD)
        ref[:k, :k] = capacitance_ref(*a, p_diag=case["pd"][b], tmax=T)
        # S_ij = sum_c |U_ic| |U_jc| / D_c: the same form on |U|
        D = case["pd"][b] + st.sigma + row_rho(lb, ub, rho[b], st)
        Ua = np.zeros((k_ld, n))
        Ua[:case["tlen"][b]] = np.sqrt(case["ps"][b]) * np.abs(a[0])
        Ua[T:k] = np.sqrt(row_rho(lg, ug, rho[b], st))[:, None] * np.abs(Cg)
        S = (Ua / D) @ Ua.T + np.eye(k_ld)
        d = np.abs(Mh[b].astype(LD) - ref).astype(np.float64)
        assert np.all(d[low] <= N * U64 * S[low]), (name, b, float(d[low].max()))
        mmax = np.abs(ref).max()
        pos = low & (S > 0)   # (S_ij = 0 in the padding: both sides are exactly 0 there)
        assert not d[low & ~pos].any()
        worst_s = max(worst_s, float((d[pos] / (U64 * S[pos])).max()))
        worst_m = max(worst_m, float(d[low].max() / (U64 * float(mmax))))
        mod = np.eye(k_ld)
        mod[:k, :k] = capacitance_ref(*a, p_diag=case["pd"][b], tmax=T, dtype=np.float64)
        worst_model = max(worst_model, float(np.abs(mod - ref).astype(np.float64)[low].max() / (U64 * float(mmax))))
    print("CAPACITANCE %-32s worst |M - ref| = %.2f u S_ij = %.2f u max|M| (float64 numpy model: %.2f u max|M|; bar N = %d)"
          % (name, worst_s, worst_m, worst_model, N))


# ---- 2. the ADMM iterates --------------------------------------------------------------------

ITER_CASES, STOP_CASE, STOP, D = wc.ITER_CASES, wc.STOP_CASE, wc.STOP, wc.DATES
_cache = {}


def _case(window, kind, mg, stride):
    key = (window, kind, mg, stride)
    if key not in _cache:
        _cache[key] = dict(case=wc.iter_case(window, kind, mg, stride), runs={})
    return _cache[key]


def _state(qb, ws):
    n, mg, p = qb.n, qb.mg, ws.mg_pad
    torch.cuda.synchronize()
    z, y = ws.z.cpu().numpy(), ws.y.cpu().numpy()
    return dict(x=ws.x[:, :n].cpu().numpy().copy(), Px=ws.Px[:, :n].cpu().numpy().copy(),
                z=np.concatenate([z[:, :mg], z[:, p:p + n]], 1), y=np.concatenate([y[:, :mg], y[:, p:p + n]], 1),
                iters=ws.iters.cpu().numpy().copy(), status=ws.status.cpu().numpy().copy(),
                rho=ws.rho.cpu().numpy().copy())


def _run(device, entry, form, settings):
    """One solve_lowrank on the direct route with the caller flags at their defaults; asserts the
    kernels that ran; returns (state, result, Settings, the initial rho)."""
    case = entry["case"]
    qb, lr, _ = wc.to_device(case, device)
    _check_inputs(case, qb, lr)
    gp = None
    if form == "grouped-unfused":   # one CU: a single group of 12 dates, ragged against GMAX = 16
        gp = engine.GroupPlan(case["rows"], case["tlen"], device, cus=1)
        assert gp.ok and gp.sizes.tolist() == [D]
    st = engine.Settings(**settings)
    ws = engine.Workspace(qb, dense=False)
    assert not engine._band_applies(qb, lr)
    route = engine.lowrank_route(qb, lr, ws, gp, st, polish=False)
    assert (route.capacitance, route.admm, route.band) == ("direct", form, False)
    rho0 = wc.initial_rho(case, st)
    res = engine.solve_lowrank(qb, lr, st, ws=ws, polish=False, groups=gp)
    state = _state(qb, ws)
    assert res.capacitance == "direct" and ws.gcap_groups is None and ws.sweep_admm is None and ws.band_shape is None
    return state, res, st, rho0


def _references(entry, st, rho, iters=None, model=True):
    key = (rho.tobytes(), repr(dataclasses.astuple(st)), iters, model)
    if key not in entry["runs"]:
        entry["runs"][key] = wc.references(entry["case"], st, rho, iters, model=model)
    return entry["runs"][key]


def _dist(rows, ref, k):
    return max(rel_dist(rows[b], getattr(ref[b], k)) for b in range(len(ref)))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("window,kind,mg,stride", ITER_CASES)
def test_direct_route_iterates(device, window, kind, mg, stride, form):
    entry = _case(window, kind, mg, stride)
    state, res, st, rho0 = _run(device, entry, form, {**FIXED, "max_iter": ITERS})
    assert res.refactors == 0
    # the kernel's own rho (k_init_state's block sum) is the host formula's to rounding; the references run at it
    assert np.abs(state["rho"] / rho0 - 1.0).max() <= 1e-12
    ref, mod = _references(entry, st, state["rho"], ITERS)
    out = {k: (_dist(state[k], ref, k), _dist([getattr(m, k) for m in mod], ref, k)) for k in VECS}
    tag = f"{window} {kind} mg{mg} s{stride} {form}"
    print("ITERATES %-58s " % tag + "  ".join("%s %.1e/%.1e" % (k, *out[k]) for k in VECS))
    assert np.all(state["iters"] == ITERS) and np.all(state["status"] == _lib.PQ_MAX_ITER)
    assert all(r.iters == ITERS and r.status == "max_iter" for r in ref)
    for k in VECS:
        dk, dm = out[k]
        assert dm >= 1e-13, (tag, k, dm)   # (the floor below decides nothing)
        assert dk <= 10.0 * dm + 1e-14, (tag, k, dk, dm)
        if k != "Px":
            assert dk <= 1e-6, (tag, k, dk)


# ---- 3. stop rule and adaptive rho -----------------------------------------------------------

ADAPT = {**FIXED, "adapt_interval": 4, "adapt_tol": 1.5, "max_iter": 12}


@pytest.mark.parametrize("form", FORMS)
def test_direct_route_stop_rule_counts(device, form):
    entry = _case(*STOP_CASE)
    state, res, st, rho0 = _run(device, entry, form, STOP)
    ref, _ = _references(entry, st, state["rho"], model=False)
    edge = stop_edge(ref)
    it_ref = np.array([r.iters for r in ref])
    print("STOP %s: reference iterations %d..%d, nearest residual/eps to 1: %.2e" % (form, it_ref.min(), it_ref.max(), edge))
    assert edge >= 1e-3, edge
    assert it_ref.min() >= st.min_iter and len(np.unique(it_ref)) > 4 and it_ref.max() < st.max_iter
    assert np.array_equal(state["iters"], it_ref), (state["iters"], it_ref)
    assert np.array_equal(state["status"], np.array([STATUS[r.status] for r in ref]))


@pytest.mark.parametrize("form", FORMS)
def test_direct_route_adaptive_rho(device, form):
    entry = _case(*STOP_CASE)
    if "rho0" not in entry:   # the initial rho: ws.rho after a run without adaptation
        entry["rho0"] = _run(device, entry, "per-problem", {**FIXED, "max_iter": 1})[0]["rho"]
    rho0 = entry["rho0"]
    state, res, st, _ = _run(device, entry, form, ADAPT)
    ref, mod = _references(entry, st, rho0)
    assert res.refactors > 0
    rho_ref = np.array([r.rho for r in ref])
    assert np.all(rho_ref != rho0)
    assert np.array_equal(state["iters"], np.array([r.iters for r in ref])), state["iters"]
    assert np.array_equal(state["status"], np.array([STATUS[r.status] for r in ref])), state["status"]
    refactors_ref = sum(sum(1 for _, rn, r0 in r.cands if rn > r0 * st.adapt_tol or rn < r0 / st.adapt_tol) for r in ref)
    assert res.refactors == refactors_ref, (res.refactors, refactors_ref)
    d_model = np.abs(np.array([m.rho for m in mod]) / rho_ref - 1.0).max()
    d_kernel = np.abs(state["rho"] / rho_ref - 1.0).max()
    print("ADAPT %s: rho d_kernel %.1e d_model %.1e refactors %d" % (form, d_kernel, d_model, res.refactors))
    assert d_kernel <= 10.0 * d_model, (d_kernel, d_model)


# ---- 4. free rows and box-less batches -------------------------------------------------------

FREE_WINDOWS = {"n282-T150-uncentred": (282, 150, False), "n300-T60-centred": (300, 60, True)}


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("ridge", [0.0, 0.05])
@pytest.mark.parametrize("kind", ["free", "nobox"])
@pytest.mark.parametrize("window", list(FREE_WINDOWS))
def test_free_rows_and_boxless_batches_are_certified(device, window, kind, ridge, grouped):
    """A box row with both sides infinite takes rho_min, so with p_diag = 0 its D_c = sigma + rho_min
    = 2e-6 next to rows at sigma + rho ~ 1e-2 .. 1; a batch without a box has that D on every asset.
    The float64 model of the kernels' algebra (admm_woodbury_diag_f64, CPU) loses the ADMM iterate
    there: after 7 iterations x is off the longdouble model by 5.8e-2 (free rows, uncentred
    282 x 150), 2.2e-4 / 3.3e-5 (no box, uncentred / centred 300 x 60) and 5.6e-8 (free rows,
    centred); with a ridge of 5 % of mean diag P by 4.5e-10 .. 9.9e-8.  At the default stop
    (eps 2e-3) the model still stops where the reference does (16 .. 21 iterations; one date of the
    free uncentred batch at 26 against 21), 1.4e-1 .. 2.5e-5 off in x.

    Measured on an MI355X, default settings, polish on, 6 dates: every date of every case is SOLVED
    and the polished point passes the KKT certificate (tests/kkt.py) inside the bars of
    tests/test_out_record_gpu.py, prim 1e-9, stat / comp / dual 1e-8: the polish solves the reduced
    KKT system of the active set the ADMM point predicts and does not go through D^-1.  Observed
    (worst over dates and over the per-date / grouped forms): ADMM iterations 17 .. 30 (free,
    ridge 0, uncentred: 20 .. 30 against the reference's 21), prim <= 5e-15, stat <= 1.4e-10
    (centred free rows; <= 7.7e-12 elsewhere), comp <= 5e-16, dual 0.  So the window form stays
    applicable to these batches, and this test is what holds it to that.

    (The box-less centred batch takes q = -P w: with a linear term outside range(P), rank P < n and
    no box the problem is unbounded below, and no route has an answer to certify.)"""
    from tests.test_out_record_gpu import Host, _certificate
    n, T, centred = FREE_WINDOWS[window]
    case = wc.window_case(kind, n, T, 6, 1, centred, 1, ridge=ridge)
    qb, lr, _ = wc.to_device(case, device)
    _check_inputs(case, qb, lr)
    if kind == "free":
        both = np.isinf(case["lb"]) & np.isinf(case["ub"])
        assert both.any() and not both.all() and not engine._band_applies(qb, lr)
    else:
        assert qb.lb is None and qb.ub is None and not qb.has_box
    gp = engine.GroupPlan(case["rows"], case["tlen"], device) if grouped else None
    st = engine.Settings()
    ws = engine.Workspace(qb, dense=False)
    assert engine.lowrank_applicable(qb, lr)
    res = engine.solve_lowrank(qb, lr, st, ws=ws, groups=gp)
    torch.cuda.synchronize()
    assert (res.capacitance == "direct") == (kind == "free")   # (no box: one D for every asset, band or group)
    host = Host(qb, lr)
    x, y, zb = (t.cpu().numpy().copy() for t in (res.x, res.y, res.z_box))
    status, iters = res.status.cpu().numpy(), res.iters.cpu().numpy()
    worst = dict(prim=0.0, stat=0.0, comp=0.0, dual=0.0)
    for i in range(host.B):
        C, lg, ug = host.rows_of(i)
        lb, ub = host.box_of(i)
        c = _certificate(host.P_eff(i), host.q[i], x[i], y[i], zb[i], C, lg, ug, lb, ub)
        worst = {k: max(worst[k], c[k]) for k in worst}
    print("FREE %s %s ridge %.2f %s: %s, status %s, iterations %d..%d, " % (
        window, kind, ridge, "grouped" if grouped else "per-date", res.capacitance, status.tolist(), iters.min(),
        iters.max()) + "  ".join("%s %.1e" % kv for kv in worst.items()))
    assert np.all(status == _lib.PQ_SOLVED), status
    assert worst["prim"] <= 1e-9 and max(worst["stat"], worst["comp"], worst["dual"]) <= 1e-8, worst
    if kind == "free":
        assert (np.abs(x[:, both[0]]) > 0).any()
