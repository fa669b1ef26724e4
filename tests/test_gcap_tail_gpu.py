"""The tail form of the group-capacitance ADMM (admm_gcap.hip, k_admm_gcap<MGC, 2, 1>): groups
of 17 .. 20 dates run dates 0 .. 15 on the MFMA and the dates past 16 on the vector pipe in the
two passes over the union rows; pass 2 deals the asset blocks over all eight waves.

* Iterates after ITERS = 7 iterations against the dense extended-precision model of
  tests/admm_reference.py, with the bars of tests/test_admm_iterates_gpu.py (d_kernel <=
  10 d_model + 1e-14 for x, z, y, Px; <= 1e-6 outright for x, z, y), the form that ran asserted
  through pq_gcap_form.  One fixed rho (rho0 = 0.01, no scale-aware start), so that the CPU
  test below can state the yardstick without a device.
* The same solve with PQ_GCAP_TAIL=0 (both column blocks on the MFMA) in the same process:
  equal status and iteration counts, every vector within 10 d_model of the other form.
* test_reference_bar_holds (CPU): 10 d_model <= 1e-6 for x, z, y on every case, by the
  reference alone.
* Inactive dates of a 19-date group (the three tail dates SOLVED; then only they active):
  bit-identical state for the inactive ones, the others iterate as in the all-active run.
* Adaptive rho and the stop rule on a group of 19: refactorisations, iteration counts and
  status equal those of the MFMA form.

Cases: centred windows.  n = 300 (9 x 32 + 12 assets: a ragged last asset block and one more
block than the eight waves of pass 2) with T = 60 at stride 3; n = 282 with T = 150 at stride 1
(unions that are no multiple of 16 rows).  Plans are built for one CU, so the date count sets
the group sizes: 33 -> 17 + 16 (tail 1, and a group without a tail inside a tail-form launch),
39 -> 20 + 19 (tail 4 and 3), 19, 20, and 21 (the first size that takes the MFMA form).
General rows: none (q = -50 mu), the budget, the budget with two sector caps.

d_model by the reference alone, worst over the cases: x 2.9e-8 (n282-T150-s1-D20-mg1), z 1.8e-9,
y 1.8e-8 (n300-T60-s3-D19-mg3); box only 3e-15 .. 3e-14.  (Two sector caps on the 282 x 150
windows give x 1.03e-7, over the 1e-7 the CPU test asks for: that case carries the caps on the
stride-3 windows instead.)
Measured on an MI355X (profiles/r09_tail_pytest_tail.txt), d_kernel / d_model:
  tail form vs the reference      x 2.6e-9 / 1.7e-8   z 3.4e-10 / 1.8e-9   y 5.1e-8 / 1.3e-8 (3.9)   Px 3.4e-4 / 7.6e-5 (4.5)
  tail form vs the MFMA form      x 3.6e-9 / 3.9e-8   z 2.9e-10 / 1.8e-9   y 5.5e-8 / 9.1e-9 (6.0)   Px 3.0e-4 / 5.1e-5 (5.9)
  box only: 6e-15 .. 1.2e-13 / 3e-15 .. 3e-14 (3.9); stop / rho case: 174 date-refactorisations,
  157 .. 283 iterations per date, equal in both forms.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from porqua_amd.synthetic import factor_panel
from tests.admm_reference import admm_dense_ref, admm_woodbury_f64, LD, rel_dist

ITERS = 7
VECS = ("x", "z", "y", "Px")
RHO0 = 0.01
# name: n, T, stride, D, ub, (budget, caps), group sizes of the 32-date plan, form (3 = tail)
CASES = {
    "n300-T60-s3-D33-mg1": (300, 60, 3, 33, 0.2, (True, 0), [17, 16], 3),
    "n300-T60-s3-D39-mg0": (300, 60, 3, 39, 0.2, (False, 0), [20, 19], 3),
    "n300-T60-s3-D19-mg3": (300, 60, 3, 19, 0.2, (True, 2), [19], 3),
    "n282-T150-s1-D20-mg1": (282, 150, 1, 20, 1.0, (True, 0), [20], 3),
    "n300-T60-s3-D21-mg1": (300, 60, 3, 21, 0.2, (True, 0), [21], 2),
}
_cache = {}


def _settings(**kw):
    from porqua_amd import engine
    base = dict(polish=0, eps_abs=1e-12, eps_rel=1e-12, eps_grouped=0.0, adapt_interval=0, max_iter=ITERS,
                rho0_rel=0.0, rho0=RHO0, rho0_qrel=0.0)
    return engine.Settings(**{**base, **kw})


def _host_inputs(case):
    """The problem of tests/test_gcap_gpu.py::_problem in numpy (what the kernels read back as
    their inputs on the device; the GPU test asserts that the two agree)."""
    from porqua_amd import engine
    n, T, stride, D, ub, (budget, caps), _, _ = CASES[case]
    ends = list(range(T + 5, T + 5 + D * stride, stride))
    dates, R, _, sec = factor_panel(max(ends) + 1, n)
    rows, tlen = engine.window_rows(dates, dates[ends], T)
    rows, tlen = np.asarray(rows), np.asarray(tlen)
    R = np.asarray(R, dtype=np.float64)[:, :n]
    mu = np.stack([R[rows[b, :tlen[b]]].mean(0) for b in range(D)])
    Cg = np.concatenate([np.ones((int(budget), n))] + [(sec == g).astype(float)[None, :] for g in range(caps)]) \
        if budget or caps else np.zeros((0, n))
    lg = np.array([1.0] * int(budget) + [-np.inf] * caps)
    ug = np.array([1.0] * int(budget) + [0.3] * caps)
    q = np.zeros((D, n)) if budget else -50.0 * mu
    return dict(n=n, mg=Cg.shape[0], B=D, R=R, rows=rows, tlen=tlen, mu=mu, ps=2.0 / (tlen.astype(np.float64) - 1.0),
                pd=None, q=q, Cg=Cg, lg=lg, ug=ug, lb=np.zeros(n), ub=np.full(n, ub), rho=np.full(D, RHO0))


def _reference(case, inp, st):
    """(dense longdouble reference, float64 Woodbury model) per date, once per case."""
    if case not in _cache:
        ref, mod = [], []
        for b in range(inp["B"]):
            X = inp["R"][inp["rows"][b, :inp["tlen"][b]]]
            Xc = X - inp["mu"][b]
            Xl = X.astype(LD) - inp["mu"][b].astype(LD)
            a = (inp["q"][b], inp["Cg"], inp["lg"], inp["ug"], inp["lb"], inp["ub"], inp["rho"][b], st, ITERS)
            ref.append(admm_dense_ref(LD(inp["ps"][b]) * (Xl.T @ Xl), *a))
            mod.append(admm_woodbury_f64(Xc, inp["ps"][b], *a))
        _cache[case] = (ref, mod)
    return _cache[case]


def _dist(rows, ref, k):
    return max(rel_dist(rows[b], getattr(ref[b], k)) for b in range(len(ref)))


def _d_model(case):
    ref, mod = _reference(case, _host_inputs(case), _settings())
    return {k: _dist([getattr(m, k) for m in mod], ref, k) for k in VECS}


@pytest.mark.parametrize("case", list(CASES))
def test_reference_bar_holds(case):
    """By the reference alone: the 10 d_model bar stays under 1e-6 for x, z and y."""
    dm = _d_model(case)
    print("D_MODEL %-24s " % case + "  ".join("%s %.1e" % (k, dm[k]) for k in VECS))
    for k in ("x", "z", "y"):
        assert 10.0 * dm[k] <= 1e-6, (case, k, dm[k])


# ---- on the device ---------------------------------------------------------------------------

def _problem_case(device, case):
    from porqua_amd import engine
    from tests.test_gcap_gpu import _problem
    n, T, stride, D, ub, (budget, caps), sizes, form = CASES[case]
    qb, lr, gp = _problem(device, n, T, D, ub, stride, centred=True, budget=budget, caps=caps, cus=1)
    if not budget:
        qb.q = (-lr.mu * 50.0).contiguous()
    assert qb.mg == int(budget) + caps
    g32 = gp.gcap_plan()
    assert gp.ok and g32 is not gp and g32.sizes.tolist() == sizes, g32.sizes.tolist()
    return qb, lr, gp, g32


def _solve(device, case, tail, monkeypatch, st=None, keep=None):
    """One solve of the case through the group capacitance; tail: the form asked for (the
    switch is read by the library on every call).  Returns (qb, lr, ws, res)."""
    from porqua_amd import _lib, engine
    if tail:
        monkeypatch.delenv("PQ_GCAP_TAIL", raising=False)
    else:
        monkeypatch.setenv("PQ_GCAP_TAIL", "0")
    qb, lr, gp, g32 = _problem_case(device, case)
    want = CASES[case][7] if tail else 2
    assert _lib.load().pq_gcap_form(int(g32.sizes.max()), qb.mg) == want   # the form the launch takes
    if keep is not None:   # keep the solve object (its C structs and buffers) for a second launch
        orig = engine._LowRankSolve.admm_rounds

        def spy(self, *a, **k):
            keep.append(self)
            return orig(self, *a, **k)
        monkeypatch.setattr(engine._LowRankSolve, "admm_rounds", spy)
    ws = engine.Workspace(qb, dense=False)
    res = engine.solve_lowrank(qb, lr, st or _settings(), ws=ws, polish=False, groups=gp, gcap=True)
    import torch
    torch.cuda.synchronize()
    assert res.capacitance == "group" and ws.gcap_groups is g32
    return qb, lr, ws, res


def _runs(device, case, monkeypatch):
    """(inputs, state of the tail form -- or of the form the case takes --, state with PQ_GCAP_TAIL=0)."""
    from tests.test_admm_iterates_gpu import _inputs, _state
    key = ("runs", case)
    if key not in _cache:
        qb, lr, ws, res = _solve(device, case, True, monkeypatch)
        assert res.refactors == 0
        inp, a = _inputs(qb, lr, ws), _state(qb, ws)
        qb2, lr2, ws2, res2 = _solve(device, case, False, monkeypatch)
        assert res2.refactors == 0
        _cache[key] = (inp, a, _state(qb2, ws2))
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_tail_form_iterates(device, case, monkeypatch):
    from porqua_amd import _lib
    inp, state, _ = _runs(device, case, monkeypatch)
    host = _host_inputs(case)
    # the device's inputs are the host model's (the CPU test's yardstick is this problem's)
    # (rho: the group mean of its dates' rho0, RHO0 to an ulp)
    assert np.allclose(inp["rho"], host["rho"], rtol=1e-14, atol=0.0), inp["rho"]
    assert np.array_equal(inp["rows"][:, :host["rows"].shape[1]], host["rows"])
    for k in ("R", "mu", "ps", "q", "Cg", "lg", "ug", "lb", "ub"):
        assert np.allclose(inp[k], host[k], rtol=1e-12, atol=1e-300), k
    ref, mod = _reference(case, host, _settings())
    out = {k: (_dist(state[k], ref, k), _dist([getattr(m, k) for m in mod], ref, k)) for k in VECS}
    print("ITERATES %-24s form %d  " % (case, CASES[case][7]) + "  ".join("%s %.1e/%.1e" % (k, *out[k]) for k in VECS))
    assert np.all(state["iters"] == ITERS) and np.all(state["status"] == _lib.PQ_MAX_ITER)
    assert all(r.iters == ITERS and r.status == "max_iter" for r in ref)
    for k in VECS:
        dk, dm = out[k]
        assert dk <= 10.0 * dm + 1e-14, (case, k, dk, dm)
        if k != "Px":
            assert dk <= 1e-6, (case, k, dk)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][7] == 3])
def test_tail_form_against_mfma_form(device, case, monkeypatch):
    inp, a, b = _runs(device, case, monkeypatch)
    ref, mod = _reference(case, _host_inputs(case), _settings())
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"])
    line = []
    for k in VECS:
        dm = _dist([getattr(m, k) for m in mod], ref, k)
        dk = max(float(np.abs(a[k][i] - b[k][i]).max()) / float(np.abs(np.asarray(getattr(ref[i], k), dtype=np.float64)).max())
                 for i in range(len(ref)))
        line.append("%s %.1e/%.1e" % (k, dk, dm))
        assert dk <= 10.0 * dm + 1e-14, (case, k, dk, dm)
    print("TAIL-vs-MFMA %-24s " % case + "  ".join(line))
    assert any(not np.array_equal(a[k], b[k]) for k in VECS)   # (two forms did run: another summation order)


# ---- inactive dates ---------------------------------------------------------------------------

def _second_call(c, ws, active, extra):
    """Mark ``active`` dates UNSOLVED and the others SOLVED, then launch the entry point again
    with max_iter raised by ``extra``."""
    import torch
    from porqua_amd import _lib
    stt = torch.full_like(ws.status, _lib.PQ_SOLVED)
    stt[torch.as_tensor(active, device=ws.status.device)] = _lib.PQ_UNSOLVED
    ws.status.copy_(stt)
    s2 = dataclasses.replace(c.settings, max_iter=ITERS + extra).to_c()
    _lib.check(c.admm(None, 0, ctypes.byref(s2)), "pq_admm_lr_gcap")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tail-inactive", "tail-only-active"])
@pytest.mark.parametrize("tail", [True, False], ids=["tailform", "mfmaform"])
def test_inactive_dates_untouched(device, monkeypatch, which, tail):
    """A 19-date group entered with some dates SOLVED: their x, z, y, Px, iters and status come
    back bit for bit; the active ones iterate exactly as when every date is active (the dates
    of a group share nothing but the group's rho, fixed here)."""
    from porqua_amd import _lib
    from tests.test_admm_iterates_gpu import _state
    case, EXTRA = "n300-T60-s3-D19-mg3", 3
    active = list(range(16)) if which == "tail-inactive" else [16, 17, 18]
    idle = [b for b in range(19) if b not in active]
    keep = []
    qb, lr, ws, _ = _solve(device, case, tail, monkeypatch, keep=keep)
    before = _state(qb, ws)
    assert np.all(before["status"] == _lib.PQ_MAX_ITER)
    _second_call(keep[-1], ws, active, EXTRA)
    part = _state(qb, ws)
    keep2 = []
    qb2, lr2, ws2, _ = _solve(device, case, tail, monkeypatch, keep=keep2)
    assert all(np.array_equal(before[k], _state(qb2, ws2)[k]) for k in VECS)   # (the solve is deterministic)
    _second_call(keep2[-1], ws2, list(range(19)), EXTRA)
    full = _state(qb2, ws2)
    assert np.all(full["iters"] == ITERS + EXTRA) and np.all(full["status"] == _lib.PQ_MAX_ITER)
    for k in VECS:
        assert np.array_equal(part[k][idle], before[k][idle]), (which, k)
        assert np.array_equal(part[k][active], full[k][active]), (which, k)
        assert not np.array_equal(part[k][active], before[k][active])
    assert np.all(part["iters"][idle] == ITERS) and np.all(part["status"][idle] == _lib.PQ_SOLVED)
    assert np.all(part["iters"][active] == ITERS + EXTRA) and np.all(part["status"][active] == _lib.PQ_MAX_ITER)


# ---- stop rule and rho bookkeeping --------------------------------------------------------------

@pytest.mark.gpu
def test_stop_and_rho_bookkeeping_equal_mfma_form(device, monkeypatch):
    """A group of 19 with adaptive rho and a stop the dates reach at different iterations: the
    refactorisation count, every date's iteration count and status equal the MFMA form's -- the
    tail dates' residual maxima and mu.V partials reach the per-date decision."""
    from porqua_amd import _lib
    from tests.test_admm_iterates_gpu import _state
    case = "n300-T60-s3-D19-mg3"
    st = _settings(eps_abs=1e-4, eps_rel=1e-4, min_iter=3, max_iter=400, adapt_interval=4, adapt_tol=1.5)
    out = []
    for tail in (True, False):
        qb, lr, ws, res = _solve(device, case, tail, monkeypatch, st=st)
        out.append((_state(qb, ws), res.refactors))
    (a, ra), (b, rb) = out
    print("STOP/RHO tail: refactors %d iters %s" % (ra, a["iters"].tolist()))
    assert ra > 0 and ra == rb, (ra, rb)
    assert np.all(a["status"] == _lib.PQ_SOLVED), a["status"]
    assert a["iters"].min() > st.min_iter   # no date stopped on an empty residual
    assert np.array_equal(a["iters"], b["iters"]), (a["iters"], b["iters"])
    assert np.array_equal(a["status"], b["status"])
    assert np.allclose(a["rho"], b["rho"], rtol=1e-6), (a["rho"], b["rho"])
