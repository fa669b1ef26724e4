"""The iterates of the dense ADMM kernel, k_admm<NQ, 1, 0> behind pq_admm_batched (symv_lower on
the lower triangle of K^-1, the Px recurrence, the general-row and box updates, the stop rule,
the adaptive-rho request and the refactorisation on an index list), against the dense
extended-precision model of the same iteration (tests/admm_reference.py) -- the method of
tests/test_admm_iterates_gpu.py on the dense path.

The run is engine.solve with polish = 0: pq_init_state -> pq_factor_batched (invert = 1) ->
pq_admm_batched [-> pq_factor_batched on the index list of the problems that asked for a new rho
-> pq_admm_batched ...].  Every case first asserts the entry points (res.admm_launches,
res.refactors) and the factor route (pq_factor_last_route), then reads back ws.x, ws.Px, ws.z,
ws.y, ws.iters, ws.status and ws.rho -- the kernel's own rho: rho0_rel mean diag(P_eff) from
k_init_state, floored at rho0_qrel max|q| by the engine.  The reference gets ps P + pd I formed
in longdouble from the float64 P the kernel is given.

Batches (tests/dense_cases.py::portfolio_batch), B = 5 sliding 60-row factor_panel windows:
  centred     P = the window covariance, a small linear q, SHARED rows and box
  tracking    P = X'X, q = -2 ps X'y (uncentred), PER-PROBLEM rows and boxes
p_scale (1.6 .. 2.4) and p_diag (0 .. 5 % of mean diag P) vary over the batch; mg = 4: the budget
(equality), a cap (one-sided), a band (two-sided), a row without bounds (rho_min); the box has
ordinary, fixed (lb == ub), free and one-sided variables.

Shapes, each another k_admm<NQ> instance and another edge of symv_lower (AW = 8 waves take RU = 2
rows each at a time; lanes own column pairs of 128-wide slices):
  n = 24   NQ 1; the second row of the last pair is beyond n
  n = 130  NQ 2, ld = 192 (not a multiple of 128), n % 16 = 2
  n = 300  NQ 3        n = 520  NQ 5, ld = 576        n = 900  NQ 8, ld = 960 (B = 2)

Iterates (max_iter = 7, eps 1e-12, no adaptation), for x, z and y over [general; box] and Px:

    d_kernel = max_b |kernel - ref|_inf / |ref|_inf  <=  10 d_model + 1e-14

with d_model the same distance of admm_explicit_inverse_f64 (float64, K^-1 = L^-T L^-1 formed
explicitly: the dense kernels' algebra) at run time on the same inputs; 10 is the project's
margin between summation orders.  Besides, d_kernel <= 1e-8 outright for x, z and y: the bar is
never looser than designed, and 10 d_model <= 1e-8 holds by the reference alone (asserted here
and, for the three smaller sizes, in tests/test_admm_reference.py on the CPU: d_model <= 4.7e-10
at n <= 130 and <= 1e-10 beyond, where the budget row is written 0.25 1'x = 0.25 -- see
dense_cases.portfolio_rows for that lever).  Px is the residual of the K solve scaled by
rho eq_scale; it keeps the 10 d_model bar alone (d_model 8e-10 .. 2.9e-7 on the CPU).

Stop rule (eps 1.6e-3, min_iter 3, max_iter 60): iters and status equal the reference's for every
problem; by the reference alone, checked in the test before the GPU's answer is looked at, every
iteration's rp / eps_p and rd / eps_d is >= 1e-3 away from 1 (CPU: >= 3.0e-3; 19 .. 37
iterations).

Adaptive rho (interval 4, tol 1.5, max_iter 12): res.refactors equals the reference's count and
the final ws.rho is within 10 x (the explicit-inverse model's own rho distance) + 1e-14 of the
reference's; by the reference alone every accept / reject decision is >= 1e-3 away from the
threshold and every batch refactors (CPU, n <= 300: every problem declines at iteration 4 with
rho_new / rho 0.80 .. 0.81 and accepts at 8 with 0.59 .. 0.60, against 1 / 1.5 = 0.667).  One such
case runs n = 24 with B = CUs + 1 problems cycling 8 distinct ones: the first factor and the
refactor (an index list of all B > CUs problems) both go to k_factor with invert = 1, the
production shape of a dense daily backtest; every problem of the batch is compared.

Measured on an MI355X (256 CUs), d_kernel / d_model after 7 iterations:
  n, batch        x                z                y                Px
  24  centred     2.1e-11/1.7e-11  7.7e-12/7.0e-12  2.7e-11/4.5e-11  2.8e-08/4.7e-08
  24  tracking    2.4e-11/2.5e-11  1.8e-11/1.5e-11  2.3e-11/4.9e-11  3.4e-08/7.4e-08
  130 centred     1.9e-11/2.5e-11  4.7e-11/5.2e-11  1.1e-10/1.4e-10  4.9e-08/9.1e-08
  130 tracking    2.5e-10/3.4e-10  4.7e-11/6.2e-11  1.1e-10/4.7e-10  6.8e-08/2.9e-07
  300 centred     4.2e-12/6.1e-12  1.9e-11/2.3e-11  6.9e-12/1.9e-11  2.8e-10/7.9e-10
  300 tracking    2.3e-11/2.9e-11  2.6e-11/3.2e-11  8.0e-12/2.3e-11  2.8e-10/8.2e-10
  520 centred     2.1e-11/1.4e-11  3.4e-11/2.6e-11  2.5e-11/3.3e-11  9.7e-10/1.3e-09
  520 tracking    3.1e-11/6.2e-11  3.3e-11/7.3e-11  1.1e-11/8.3e-11  3.9e-10/2.9e-09
  900 centred     4.1e-12/3.8e-12  1.1e-11/1.1e-11  3.6e-11/2.5e-11  1.2e-09/1.1e-09
  900 tracking    1.6e-11/1.6e-11  6.3e-11/4.0e-11  8.4e-12/1.8e-11  2.8e-10/6.0e-10
(worst d_kernel / d_model 1.6: z at 900 tracking and y, x at 520 / 900 centred; within the 10.)
Stop rule: every count and status equal; reference iterations 19 .. 37, nearest residual / eps to 1
3.05e-3 (520 centred), elsewhere >= 8.6e-3.  Adaptive rho: |rho / rho_ref - 1| 1.8e-11 .. 2.4e-10
against the model's 2.8e-11 .. 5.5e-10 (worst ratio 1.0; 3.3 in the 257-problem batch: 8.3e-11 /
2.5e-11); decisions >= 2.1e-2 from the threshold; every problem accepts at iteration 8, one of
520 centred and both of 900 centred also at 4 (a refactor on an index list of one or two problems,
the others' K^-1 untouched); the iterates after 12 iterations stay within 2.2 x d_model.  257
problems: 257 refactorisations in one round, route 0.
"""
import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from tests import dense_cases
from tests.admm_reference import rel_dist

pytestmark = pytest.mark.gpu

ITERS = 7
VECS = ("x", "z", "y", "Px")
STATUS = {"solved": _lib.PQ_SOLVED, "max_iter": _lib.PQ_MAX_ITER, "unsolved": _lib.PQ_UNSOLVED}
FIXED = dict(polish=0, eps_abs=1e-12, eps_rel=1e-12, adapt_interval=0, max_iter=ITERS)
STOP = dict(polish=0, eps_abs=1.6e-3, eps_rel=1.6e-3, adapt_interval=0, min_iter=3, max_iter=60)
ADAPT = dict(polish=0, eps_abs=1e-12, eps_rel=1e-12, adapt_interval=4, adapt_tol=1.5, max_iter=12)
SHAPES = [(24, 5), (130, 5), (300, 5), (520, 5), (900, 2)]
CASES = [(n, B, batch) for n, B in SHAPES for batch in ("centred", "tracking")]
ROUTE_GEN, ROUTE_SK = 0, 1

_cases, _rho0 = {}, {}


def _case(n, B, batch):
    key = (n, B, batch)
    if key not in _cases:
        _cases[key] = dense_cases.portfolio_batch(n, B, batch == "centred")
    return _cases[key]


def _solve(device, case, settings, B=None):
    """engine.solve of problems b % case B on the dense path; returns (result, state read back, route)."""
    n, D = case["n"], case["B"]
    B = B or D
    cyc = np.arange(B) % D
    nc = case["Cg"].shape[0]
    pick = cyc if nc > 1 else np.zeros(1, dtype=int)
    qb = engine.QPBatch(n, B, 4, device=device, shared_constraints=nc == 1, has_box=True,
                        P=torch.empty(0, dtype=torch.float64, device=device))
    ld = qb.ld

    def dev(a, fill=0.0):   # (..., n) -> (..., ld) on the device
        p = np.full(a.shape[:-1] + (ld,), fill)
        p[..., :n] = a
        return torch.from_numpy(p).to(device)

    Pp = np.zeros((B, ld, ld))
    Pp[:, :n, :n] = case["P"][cyc]
    qb.P = torch.from_numpy(Pp).to(device)
    qb.q = dev(case["q"][cyc])
    qb.p_scale = torch.from_numpy(case["ps"][cyc]).to(device)
    qb.p_diag = torch.from_numpy(case["pd"][cyc]).to(device)
    qb.Cg = dev(case["Cg"][pick])
    qb.lg, qb.ug = torch.from_numpy(case["lg"][pick]).to(device), torch.from_numpy(case["ug"][pick]).to(device)
    qb.lb, qb.ub = dev(case["lb"][pick], -np.inf), dev(case["ub"][pick], np.inf)
    ws = engine.Workspace(qb)
    res = engine.solve(qb, settings, ws=ws)
    torch.cuda.synchronize()
    route = int(_lib.load().pq_factor_last_route())
    mg, p = qb.mg, ws.mg_pad
    z, y = ws.z.cpu().numpy(), ws.y.cpu().numpy()
    state = dict(x=ws.x[:, :n].cpu().numpy(), Px=ws.Px[:, :n].cpu().numpy(),
                 z=np.concatenate([z[:, :mg], z[:, p:p + n]], 1), y=np.concatenate([y[:, :mg], y[:, p:p + n]], 1),
                 iters=ws.iters.cpu().numpy(), status=ws.status.cpu().numpy(), rho=ws.rho.cpu().numpy())
    return res, state, route


def _initial_rho(device, case, key):
    """The kernel's own initial rho (ws.rho after a run that does not adapt), one solve per case."""
    if key not in _rho0:
        st = engine.Settings(**{**FIXED, "max_iter": 1})
        res, state, _ = _solve(device, case, st)
        assert res.admm_launches == 1 and res.refactors == 0
        # k_init_state's mean diagonal and the engine's floor, against the host's arithmetic
        assert np.allclose(state["rho"], dense_cases.initial_rho(case, st), rtol=1e-12, atol=0.0)
        assert state["rho"].max() / state["rho"].min() > 1.05
        _rho0[key] = state["rho"].copy()
    return _rho0[key]


def _dist(rows, ref, k, cyc):
    return max(rel_dist(rows[b], getattr(ref[d], k)) for b, d in enumerate(cyc))


@pytest.mark.parametrize("n,B,batch", CASES)
def test_dense_iterates(device, n, B, batch):
    case = _case(n, B, batch)
    st = engine.Settings(**FIXED)
    res, state, route = _solve(device, case, st)
    assert res.admm_launches == 1 and res.refactors == 0 and route == ROUTE_SK
    assert np.all(state["iters"] == ITERS) and np.all(state["status"] == _lib.PQ_MAX_ITER)
    assert np.array_equal(state["rho"], _initial_rho(device, case, (n, B, batch)))
    ref, mod = dense_cases.references(case, st, state["rho"])
    assert all(r.iters == ITERS and r.status == "max_iter" for r in ref + mod)
    cyc = np.arange(B)
    out = {k: (_dist(state[k], ref, k, cyc), _dist([getattr(m, k) for m in mod], ref, k, cyc)) for k in VECS}
    print("ITERATES n=%d %-8s " % (n, batch) + "  ".join("%s %.1e/%.1e" % (k, *out[k]) for k in VECS))
    for k in VECS:
        dk, dm = out[k]
        if k != "Px":   # by the reference alone: the bar is never looser than the 1e-8 it was designed for
            assert 10.0 * dm <= 1e-8, (k, dm)
            assert dk <= 1e-8, (k, dk)
        assert dk <= 10.0 * dm + 1e-14, (k, dk, dm)


@pytest.mark.parametrize("n,B,batch", CASES)
def test_dense_stop_rule_counts(device, n, B, batch):
    case = _case(n, B, batch)
    st = engine.Settings(**STOP)
    rho0 = _initial_rho(device, case, (n, B, batch))
    ref, _ = dense_cases.references(case, st, rho0, model=False)
    # by the reference alone: no stop decision rests on rounding
    edge = dense_cases.stop_edge(ref)
    it_ref = np.array([r.iters for r in ref])
    print("STOP n=%d %s: reference iterations %d..%d, nearest residual/eps to 1: %.2e"
          % (n, batch, it_ref.min(), it_ref.max(), edge))
    assert edge >= 1e-3, edge
    assert it_ref.min() >= st.min_iter and it_ref.max() < st.max_iter
    res, state, route = _solve(device, case, st)
    assert res.admm_launches == 1 and res.refactors == 0 and route == ROUTE_SK
    assert np.array_equal(state["rho"], rho0)
    assert np.array_equal(state["iters"], it_ref), (state["iters"], it_ref)
    assert np.array_equal(state["status"], np.array([STATUS[r.status] for r in ref]))


def _adaptive(device, case, key, B, route_want):
    st = engine.Settings(**ADAPT)
    rho0 = _initial_rho(device, case, key)
    ref, mod = dense_cases.references(case, st, rho0)
    # by the reference alone: no accept / reject decision rests on rounding, and the batch refactors
    edge = dense_cases.adapt_edge(ref, st)
    accepted = [[it for it, rn, rho in r.cands if rn > rho * st.adapt_tol or rn < rho / st.adapt_tol] for r in ref]
    assert edge >= 1e-3, edge
    assert all(len(r.cands) == 2 for r in ref) and any(accepted)
    cyc = np.arange(B) % case["B"]
    res, state, route = _solve(device, case, st, B=B)
    rounds = {it for a in accepted for it in a}
    assert res.refactors == sum(len(accepted[d]) for d in cyc) and res.admm_launches == 1 + len(rounds)
    assert route == route_want, route
    assert np.array_equal(state["iters"], np.array([ref[d].iters for d in cyc]))
    assert np.array_equal(state["status"], np.array([STATUS[ref[d].status] for d in cyc]))
    rho_ref = np.array([r.rho for r in ref])
    assert np.all(rho_ref != rho0)
    d_model = np.abs(np.array([m.rho for m in mod]) / rho_ref - 1.0).max()
    d_kernel = np.abs(state["rho"] / rho_ref[cyc] - 1.0).max()
    out = {k: (_dist(state[k], ref, k, cyc), _dist([getattr(m, k) for m in mod], ref, k, np.arange(case["B"])))
           for k in VECS}
    print("ADAPT n=%d B=%d: edge %.2e accepted at %s, rho d_kernel %.1e d_model %.1e refactors %d  "
          % (case["n"], B, edge, sorted(rounds), d_kernel, d_model, res.refactors)
          + "  ".join("%s %.1e/%.1e" % (k, *out[k]) for k in VECS))
    assert d_kernel <= 10.0 * d_model + 1e-14, (d_kernel, d_model)
    # the iterates after the refactorisation (every problem: those whose K^-1 a refactor on an index
    # list must leave alone, and those it must renew), on the bar of test_dense_iterates
    for k in VECS:
        dk, dm = out[k]
        assert dk <= 10.0 * dm + 1e-14, (k, dk, dm)


@pytest.mark.parametrize("n,B,batch", CASES)
def test_dense_adaptive_rho(device, n, B, batch):
    _adaptive(device, _case(n, B, batch), (n, B, batch), B, ROUTE_SK)


def test_dense_adaptive_rho_more_problems_than_cus(device):
    """B = CUs + 1: the first factor and the refactor on the index list both run k_factor with invert = 1."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    _adaptive(device, _case(24, 8, "tracking"), (24, 8, "tracking"), cus + 1, ROUTE_GEN)
