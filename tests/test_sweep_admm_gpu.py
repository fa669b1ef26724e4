"""The risk-aversion sweep's ADMM kernel (admm_sweep.hip, engine.SweepPlan) against the
grouped kernel it replaces (k_admm_grp's fused form):

  * iterates: after a fixed number of iterations (max_iter) x, z, y and the general rows agree
    to rounding -- same updates, same rhs, only the summation order of the window passes
    differs;
  * stops: with the sweep's loose ADMM stop the iteration counts and statuses agree, and the
    polished answers are the same optimum;
  * ragged shapes: n not a multiple of the 256-asset chunk, dates with 40 and 70 risk
    aversions (groups of 40, and 64 + 6), and a group partly solved before the call.
The optima themselves are pinned against the oracle at the config-5 shape by
tests/test_large_n_gpu.py and tests/test_full_configs_gpu.py (src/optimization.py:168-174)."""
import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.sweep import SWEEP_SETTINGS, MeanVarianceSweep
from porqua_amd.synthetic import factor_panel

pytestmark = pytest.mark.gpu


def _sweep(n, dates, lambdas, settings, device, use_kernel, per_date=False, factor="chol"):
    T, stride = 252, 21
    d_all, R, _, _ = factor_panel(T - 1 + stride * dates, n)
    ends = np.arange(T - 1, T - 1 + stride * dates, stride)
    rows, tlen = engine.window_rows(d_all, d_all[ends], T)
    pan = engine.Panel(R, device=device)
    sw = MeanVarianceSweep(pan, rows, tlen, lambdas, settings=settings, factor=factor)
    sp = sw.sp
    if not use_kernel:
        sw.sp = None
    if per_date:   # no groups at all: pq_admm_lr_batched, one workgroup per problem
        sw.sp = sw.gp = None
    res, meta = sw.solve()
    torch.cuda.synchronize()
    # which kernel ran: without this a sweep plan that does not apply (PQ_SWEEP_ADMM=0, a shape
    # rule) puts both legs of a parity test on k_admm_grp, which then agrees with itself
    assert meta["factor"] == factor
    if use_kernel and not per_date:
        assert sp is not None and sw.ws.sweep_admm is sp
    else:
        assert getattr(sw.ws, "sweep_admm", None) is None
    return sw, res


def _state(sw, res):
    ws = sw.ws
    return (res.x.cpu().numpy().copy(), ws.z.cpu().numpy().copy(), ws.y.cpu().numpy().copy(),
            res.iters.cpu().numpy().copy(), res.status.cpu().numpy().copy())


def _check_iterates(device, n, L, factor):
    lambdas = np.logspace(-1, 2, L)
    st = engine.Settings.from_params({**SWEEP_SETTINGS, "polish": 0, "max_iter": 9, "eps_grouped": 0.0,
                                    "eps_abs": 1e-12, "eps_rel": 1e-12})
    sw_a, ra = _sweep(n, 3, lambdas, st, device, True, factor=factor)
    sw_b, rb = _sweep(n, 3, lambdas, st, device, False, factor=factor)
    sw_c, rc = _sweep(n, 3, lambdas, st, device, False, per_date=True, factor=factor)
    assert sw_a.sp is not None and sw_a.sp.ngroups == 3 * ((L + 63) // 64)
    assert sw_a.ws.sweep_admm is sw_a.sp and getattr(sw_b.ws, "sweep_admm", None) is None
    assert ra.capacitance == rb.capacitance == rc.capacitance == ("eig" if factor == "eig" else "band")
    xa, za, ya, ia, sa = _state(sw_a, ra)
    xb, zb, yb, ib, sb = _state(sw_b, rb)
    xc, zc, yc, _, _ = _state(sw_c, rc)
    assert np.array_equal(ia, ib) and np.array_equal(sa, sb), (np.unique(ia), np.unique(ib))
    assert np.all(sa == _lib.PQ_MAX_ITER)
    for a, b, c in ((xa, xb, xc), (za, zb, zc), (ya, yb, yc)):
        sc = np.maximum(np.abs(b).max(1), 1e-300)
        d_new = np.abs(a - b).max(1) / sc                  # per problem, relative
        d_ref = np.abs(b - c).max(1) / sc
        assert d_new.max() <= 10.0 * d_ref.max() + 1e-14, (d_new.max(), d_ref.max())
        assert np.median(d_new) <= 10.0 * np.median(d_ref) + 1e-14, (np.median(d_new), np.median(d_ref))
        assert d_new.max() <= 1e-6, d_new.max()


@pytest.mark.parametrize("n,L", [(700, 40), (520, 70)])
def test_sweep_kernel_iterates_match_grouped_kernel(device, n, L):
    """Fixed iteration budget, no polish: the sweep kernel's iterates agree with the grouped
    kernel's as closely as the grouped kernel's agree with the per-problem kernel's
    (pq_admm_lr_batched) -- three summation orders of the same iteration, whose rounding the
    capacitance solve amplifies (cond(M_b) grows with the risk aversion)."""
    _check_iterates(device, n, L, "chol")


def test_sweep_kernel_iterates_match_grouped_kernel_eigen_capacitance(device):
    """The same with M_b^-1 formed from the per-date eigendecomposition (factor = 'eig', the
    default from 192 risk aversions per date): k_sw_mid reads the eigen form's full symmetric
    M^-1 instead of the Cholesky inverse's lower triangle.  n = 282: a second 256-asset chunk
    of one full 16-asset sub-chunk and a ragged 10; L = 192: three full groups per date."""
    _check_iterates(device, 282, 192, "eig")


def test_sweep_kernel_solves_like_grouped_kernel(device):
    """The sweep's own settings (loose stop, grouped polish): same iteration counts up to a
    stop decided within rounding, same certified optima."""
    lambdas = np.logspace(-1, 2, 64)
    st = engine.Settings.from_params(SWEEP_SETTINGS)
    sw_a, ra = _sweep(900, 4, lambdas, st, device, True)
    sw_b, rb = _sweep(900, 4, lambdas, st, device, False)
    assert sw_a.ws.sweep_admm is sw_a.sp and getattr(sw_b.ws, "sweep_admm", None) is None
    xa, _, _, ia, sa = _state(sw_a, ra)
    xb, _, _, ib, sb = _state(sw_b, rb)
    assert np.all(sa == _lib.PQ_SOLVED) and np.all(sb == _lib.PQ_SOLVED)
    assert np.mean(ia == ib) >= 0.95, (ia, ib)
    assert np.abs(xa - xb).max() <= 1e-7, np.abs(xa - xb).max()


def test_sweep_kernel_skips_solved_problems(device):
    """Problems already solved when the kernel starts keep their state (the polish hand-back
    resumes ADMM for a subset)."""
    lambdas = np.logspace(-1, 2, 48)
    st = engine.Settings.from_params({**SWEEP_SETTINGS, "polish": 0, "max_iter": 6, "eps_grouped": 0.0,
                                    "eps_abs": 1e-12, "eps_rel": 1e-12})
    T, stride, n = 252, 21, 600
    d_all, R, _, _ = factor_panel(T - 1 + stride * 2, n)
    ends = np.arange(T - 1, T - 1 + stride * 2, stride)
    rows, tlen = engine.window_rows(d_all, d_all[ends], T)
    pan = engine.Panel(R, device=device)
    sw = MeanVarianceSweep(pan, rows, tlen, lambdas, settings=st, factor="chol")
    res, _ = sw.solve()
    torch.cuda.synchronize()
    ws = sw.ws
    assert ws.sweep_admm is sw.sp
    x0 = res.x.clone()
    it0 = res.iters.clone()
    # mark every other problem solved, resume the rest through the kernel for 6 more iterations
    done = torch.zeros_like(ws.status, dtype=torch.bool)
    done[::2] = True
    ws.status[done] = _lib.PQ_SOLVED
    ws.status[~done] = _lib.PQ_UNSOLVED
    lib = _lib.load()
    qb, lr = sw.qb, sw.lr
    s = st.to_c()
    s.max_iter = 12
    M = ws.lr_buffers(256)
    bd = engine._band_setup(qb, lr, engine._stream(), w_min=0)
    scr = sw.sp.buffer(qb, lib)
    pb, stc, lrs = qb.c_struct(), ws.c_struct(), lr.c_struct()
    import ctypes
    _lib.check(lib.pq_admm_lr_sweep(ctypes.byref(lrs), ctypes.byref(pb), ctypes.byref(stc), M["Minv"].data_ptr(), 256,
                                    256 * 256, sw.sp.gdates.data_ptr(), sw.sp.ngroups, ctypes.byref(s), 6,
                                    bd["pc"].data_ptr(), bd["pc"].stride(0), bd["r0"], bd["cc"].data_ptr(), 1,
                                    scr.data_ptr(), scr.numel(), engine._stream()), "pq_admm_lr_sweep")
    torch.cuda.synchronize()
    assert torch.equal(res.x[done], x0[done])
    assert torch.equal(ws.iters[done], it0[done])
    assert bool((ws.iters[~done] == it0[~done] + 6).all())
    assert bool((res.x[~done] - x0[~done]).abs().amax() > 0)


def test_sweep_kernel_adaptive_rho_matches_grouped_kernel(device):
    """Adaptive rho inside the sweep kernel: the rho requests (NEED_REFACTOR), the engine's
    refactorisation and the resumed iterations agree with the grouped kernel's."""
    lambdas = np.logspace(-1, 2, 24)
    st = engine.Settings.from_params({**SWEEP_SETTINGS, "polish": 0, "max_iter": 14, "eps_grouped": 0.0,
                                      "eps_abs": 1e-12, "eps_rel": 1e-12, "adapt_interval": 4,
                                      "adapt_tol": 1.5})
    sw_a, ra = _sweep(600, 2, lambdas, st, device, True)
    sw_b, rb = _sweep(600, 2, lambdas, st, device, False)
    assert sw_a.ws.sweep_admm is sw_a.sp and getattr(sw_b.ws, "sweep_admm", None) is None
    assert ra.refactors > 0 and ra.refactors == rb.refactors, (ra.refactors, rb.refactors)
    xa, _, _, ia, sa = _state(sw_a, ra)
    xb, _, _, ib, sb = _state(sw_b, rb)
    assert np.array_equal(ia, ib) and np.array_equal(sa, sb)
    # the requested rho is a ratio of residual maxima, which carry the iterates' rounding
    # differences (up to ~1e-7 relative after a few iterations, the first test above)
    rho_a, rho_b = sw_a.ws.rho.cpu().numpy(), sw_b.ws.rho.cpu().numpy()
    assert np.abs(rho_a / rho_b - 1.0).max() <= 1e-5, np.abs(rho_a / rho_b - 1.0).max()
    sc = np.maximum(np.abs(xb).max(1), 1e-300)
    assert (np.abs(xa - xb).max(1) / sc).max() <= 1e-6


def test_sweep_kernel_rejects_a_capacitance_pitch_that_is_no_multiple_of_64(device):
    """k_sw_mid reads each row of M_b^-1 in 64-column blocks, up to column 64 ceil(k / 64) - 1:
    a row pitch k_ld that is no multiple of 64 (here 200 >= k = 151) would read past the rows'
    end, so the entry point refuses it -- before any launch (the state is untouched)."""
    import ctypes
    T, n, L = 150, 282, 8
    d_all, R, _, _ = factor_panel(T + 10, n)
    rows, tlen = engine.window_rows(d_all, d_all[[T + 5]], T)
    pan = engine.Panel(R, device=device)
    st = engine.Settings.from_params({**SWEEP_SETTINGS, "polish": 0, "max_iter": 3, "eps_grouped": 0.0})
    sw = MeanVarianceSweep(pan, rows, tlen, np.logspace(-1, 1, L), settings=st, factor="chol")
    sw.solve()
    torch.cuda.synchronize()
    ws, qb, lr = sw.ws, sw.qb, sw.lr
    assert ws.sweep_admm is sw.sp and lr.tmax + qb.mg == 151
    ws.status.fill_(_lib.PQ_UNSOLVED)
    x0, it0 = ws.x.clone(), ws.iters.clone()
    lib = _lib.load()
    s = st.to_c()
    s.max_iter = 6
    bd = engine._band_setup(qb, lr, engine._stream(), w_min=0)
    scr = sw.sp.buffer(qb, lib)
    pb, stc, lrs = qb.c_struct(), ws.c_struct(), lr.c_struct()

    def call(k_ld):
        Minv = torch.eye(k_ld, dtype=torch.float64, device=device).repeat(qb.batch, 1, 1).contiguous()
        return lib.pq_admm_lr_sweep(ctypes.byref(lrs), ctypes.byref(pb), ctypes.byref(stc), Minv.data_ptr(), k_ld,
                                    k_ld * k_ld, sw.sp.gdates.data_ptr(), sw.sp.ngroups, ctypes.byref(s), 3,
                                    bd["pc"].data_ptr(), bd["pc"].stride(0), bd["r0"], bd["cc"].data_ptr(), 1,
                                    scr.data_ptr(), scr.numel(), engine._stream())
    assert call(200) == -1
    assert b"multiple of 64" in lib.pq_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws.x, x0) and torch.equal(ws.iters, it0)
    assert call(150) == -1    # (k_ld < k: the check that was there before)
    assert call(320) == -1    # (beyond the kernel's 256 rows)
