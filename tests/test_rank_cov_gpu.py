"""The rank covariances on the device: pq_rank_cov_batched (the ranking kernel, Spearman's Gram on
the FP64 tile GEMM with its epilogue, Kendall's v_mfma_i32_16x16x64_i8 Gram over day pairs built
on the fly) against the NumPy model (tests/rank_model.py), and the public interface on top of it
(engine.rank_cov, Covariance 'spearman' / 'kendall', MeanVariance on the dense route,
HierarchicalRiskParity, Backtest).

The counts and the diagonal are integers and are compared bit for bit; the bars of the
floating-point results are derived below, never fitted.  The panel has ties made on purpose, and
every kernel-case window is first checked on the host to have no constant column, so that the only
bad-input dates are those of the bad-input test.  The observed worst values stand in
profiles/rank_cov_pytest.txt."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import ref_pipeline as rp
from porqua_amd import _lib, engine
from porqua_amd.backtest import Backtest, BacktestService
from porqua_amd.builders import (OptimizationItemBuilder, SelectionItemBuilder, bibfn_box_constraints,
                                 bibfn_budget_constraint, bibfn_return_series, bibfn_selection_data)
from porqua_amd.constraints import Constraints
from porqua_amd.covariance import Covariance, cov_kendall, cov_spearman
from porqua_amd.helper_functions import isPD
from porqua_amd.optimization import HierarchicalRiskParity, MeanVariance, RiskParity
from porqua_amd.optimization_data import OptimizationData
from porqua_amd.synthetic import factor_panel
from tests import hrp_model as hm
from tests import rank_model as rm

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
OK, BAD = _lib.PQ_RANK_OK, _lib.PQ_RANK_BAD_INPUT
POISON = 1e150
KINDS = ["spearman", "kendall"]
COV = {"spearman": cov_spearman, "kendall": cov_kendall}
# (T, n): the smallest window; a very small one; 55 pairs of days, less than one k-block; 66 pairs;
# a partial second asset tile; the block edges; three asset blocks with mirrored off-diagonal tiles
# and Tp = 128; larger partial tiles; the workload's window; PQ_RANK_TMAX
CASES = [(2, 1), (3, 5), (11, 17), (12, 64), (17, 70), (64, 65), (65, 130), (100, 257), (252, 130), (512, 20)]

# the correlation: one square root (<= 1 ulp) of a product (<= 1/2 ulp) and one division: 4 ulp,
# relative.  A wrong count moves an entry by at least 1 / max(C_kk, H_kk) >= 2e-8.  Expected: bit for bit
CORR_TOL = 4 * 2.0 ** -52
# Sigma relative to sd_i sd_j, the derivation of tests/test_gerber_gpu.py (sd is the same
# expression): a two-pass FP64 window variance over T <= 1024 terms is within about (T + 4) 2^-53 =
# 1.2e-13, the two sd factors double that, a few roundings are added, and the bar is ten times that
SIGMA_TOL = 1e-12
HRP_TOL = 1e-13        # HRP weights, relative (the bar of tests/test_gerber_gpu.py)
LINK_TOL = 1e-12       # sorted single-linkage merge distances against the model's spanning tree


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- fixtures (host) ----------------------------------------------------------------------------

def _with_ties(R):
    """Ties made on purpose: every third column rounded so that values repeat, every fourth
    column exactly zero where it is small, one -0.0 beside a +0.0."""
    R = R.copy()
    R[:, 2::3] = np.round(R[:, 2::3], 3)
    Z = R[:, 1::4]
    Z[np.abs(Z) < 2e-3] = 0.0
    R[:, 1::4] = Z
    R[4, 1], R[5, 1] = 0.0, -0.0
    return R


@functools.lru_cache(maxsize=None)
def _panel():
    R = _with_ties(factor_panel(400, 257, seed=5)[1])
    R[-1] = POISON
    return R


def _kernel_rows(T):
    """The three windows of tests/test_gerber_gpu.py::_kernel_rows: consecutive rows, every other
    row, and a shorter window whose unused slots point at the poison row (a valid index: a stray
    read shows as a wrong number, never as a fault), wrapped around the panel's 399 data rows
    where T needs more (a window may hold a row twice: more ties)."""
    D = _panel().shape[0]
    m = D - 1
    short = max(2, T - 3)
    rows = np.full((3, T), D - 1, dtype=np.int32)
    rows[0] = (2 + np.arange(T)) % m
    rows[1] = (1 + 2 * np.arange(T)) % m
    rows[2, :short] = (3 + np.arange(short) + (np.arange(short) > short // 2)) % m
    return rows, np.array([T, T, short], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _model(T, n, kind, b):
    rows, lens = _kernel_rows(T)
    X = _panel()[rows[b, :lens[b]], :n]
    assert (X.max(axis=0) > X.min(axis=0)).all(), "a constant column in a kernel-case window"
    return rm.rank_cov(X, kind), X


def _run(pan, rd, td, kind, output, out=None):
    B, n = rd.shape[0], pan.n
    ld = engine.round_up(n, 64)
    if out is None:
        out = torch.full((B, ld, ld), POISON, dtype=F64, device=pan.device)
    S, status, diag = engine.rank_cov(pan, rd, td, kind=kind, output=output, out=out)
    assert S is out and status.dtype == torch.int32 and diag.dtype == F64
    assert tuple(status.shape) == (B,) and tuple(diag.shape) == (B, ld)
    torch.cuda.synchronize()
    return S.cpu().numpy(), status.cpu().numpy(), diag.cpu().numpy()


def _rel(a, ref):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(ref != 0, np.abs(a - ref) / np.abs(ref), np.abs(a)).max())


# ---- 1. the kernels -----------------------------------------------------------------------------

def test_the_panel_has_ties():
    R = _panel()[:-1]
    assert (np.diff(np.sort(R[:, 2]))[:] == 0).any() and (R[:, 1] == 0).sum() > 2
    assert np.signbit(R[5, 1]) and R[5, 1] == 0 and not np.signbit(R[4, 1]) and R[4, 1] == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,n", CASES)
def test_kernels_match_model(device, T, n, kind):
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    S, st, dg = _run(pan, rd, td, kind, "cov")
    G, stg, dgg = _run(pan, rd, td, kind, "corr")
    N, stn, dgn = _run(pan, rd, td, kind, "counts")
    assert list(st) == [OK] * 3 and list(stg) == [OK] * 3 and list(stn) == [OK] * 3
    assert np.array_equal(dg, dgg) and np.array_equal(dg, dgn)
    worst = dict(g=0.0, sigma=0.0, diag=0.0)
    for b in range(3):
        mod, X = _model(T, n, kind, b)
        assert mod.status == rm.OK
        assert np.array_equal(N[b, :n, :n], mod.counts)                 # the integers, exactly
        assert np.array_equal(dg[b, :n], mod.diag) and not dg[b, n:].any()
        Gb, Sb = G[b, :n, :n], S[b, :n, :n]
        worst["g"] = max(worst["g"], _rel(Gb, mod.corr))
        worst["sigma"] = max(worst["sigma"], float((np.abs(Sb - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
        var = X.var(axis=0, ddof=1)
        worst["diag"] = max(worst["diag"], float((np.abs(np.diag(Sb) - var) / var).max()))
        assert np.array_equal(Sb, Sb.T) and np.array_equal(Gb, Gb.T)
        assert np.array_equal(np.diag(Gb), np.ones(n))
        for M in (S[b], G[b], N[b]):                                    # the padding of a caller's out is zeroed
            assert not M[n:, :].any() and not M[:, n:].any()
        # the date alone: the same bits
        S1, st1, dg1 = _run(pan, rd[b:b + 1], td[b:b + 1], kind, "cov")
        assert st1[0] == OK and np.array_equal(S1[0], S[b]) and np.array_equal(dg1[0], dg[b])
    print(f"{kind} (T, n) = {(T, n)}: corr {worst['g']:.2e}, Sigma {worst['sigma']:.2e}, diag {worst['diag']:.2e}")
    assert worst["g"] <= CORR_TOL
    assert worst["sigma"] <= SIGMA_TOL
    assert worst["diag"] <= SIGMA_TOL


@pytest.mark.parametrize("kind", KINDS)
def test_chunks_and_repeats_are_bitwise_equal(device, kind):
    T, n = 65, 130
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    one = engine.rank_cov(pan, rd, td, kind=kind)
    two = engine.rank_cov(pan, rd, td, kind=kind, chunk_bytes=1)        # one date per chunk of the rank scratch
    three = engine.rank_cov(pan, rd, td, kind=kind)
    for a, b, c in zip(one, two, three):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not one[0][:, n:, :].any() and not one[0][:, :, n:].any()   # an allocated result: zero padding too
    empty = engine.rank_cov(pan, rd[:0], td[:0], kind=kind)
    assert empty[0].shape == (0, 192, 192) and empty[1].shape == (0,) and empty[2].shape == (0, 192)
    assert empty[0].dtype == F64 and empty[1].dtype == torch.int32 and empty[2].dtype == F64


# ---- 2. bad input -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_bad_dates_do_not_affect_their_neighbours(device, kind):
    """A constant column, a NaN, an inf and a one-row window in one batch beside two good dates:
    BAD_INPUT and a NaN block each; the good dates' bits are their solo run's."""
    T, n = 17, 20
    R = _panel()[:, :n].copy()
    R[100:100 + T, 3] = 0.25
    R[155, 2] = np.nan
    R[205, 7] = np.inf
    starts = [2, 100, 150, 40, 60, 200]
    rows = np.stack([s + np.arange(T) for s in starts]).astype(np.int32)
    lens = np.array([T, T, T, T, 1, T], dtype=np.int32)
    rows[4, 1:] = R.shape[0] - 1
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    for output in ("cov", "counts"):
        S, st, dg = _run(pan, rd, td, kind, output)
        assert list(st) == [OK, BAD, BAD, OK, BAD, BAD]
        for b in (1, 2, 4, 5):
            assert rm.rank_cov(R[rows[b, :lens[b]]], kind).status == rm.BAD_INPUT
            assert np.isnan(S[b, :n, :n]).all()
            assert not S[b, n:, :].any() and not S[b, :, n:].any()
        for b in (0, 3):
            mod = rm.rank_cov(R[rows[b]], kind)
            assert mod.status == rm.OK and np.array_equal(dg[b, :n], mod.diag)
            if output == "counts":
                assert np.array_equal(S[b, :n, :n], mod.counts)
            else:
                assert float((np.abs(S[b, :n, :n] - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()) <= SIGMA_TOL
            S1, st1, _ = _run(pan, rd[b:b + 1], td[b:b + 1], kind, output)
            assert st1[0] == OK and np.array_equal(S1[0], S[b])


# ---- 3. host argument checks: an error, nothing launched ------------------------------------------

@pytest.mark.parametrize("kind", [_lib.PQ_RANK_SPEARMAN, _lib.PQ_RANK_KENDALL])
@pytest.mark.parametrize("kw", [{"tmax": _lib.PQ_RANK_TMAX + 1}, {"tmax": 0}, {"kind": 2}, {"kind": -1}, {"mode": 3},
                                {"mode": -1}, {"stages": 0}, {"stages": 4}, {"stages": 3, "kind": _lib.PQ_RANK_SPEARMAN}, {"n": 0}, {"ldp": 19}, {"ld": 19},
                                {"ld": 32}, {"ldd": 19}, {"dg_stride": 19}, {"out_stride": 64 * 63},
                                {"null": "panel"}, {"null": "rows"}, {"null": "tlen"}, {"null": "dg"},
                                {"null": "scratch"}, {"null": "diag"}, {"null": "out"}, {"null": "status"}])
def test_host_argument_checks(device, kw, kind):
    T, n = 17, 20
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    dg = pan.window_sumsq(rd, td, pan.window_means(rd, td))
    out = torch.full((3, 64, 64), POISON, dtype=F64, device=device)
    status = torch.full((3,), 7, dtype=torch.int32, device=device)
    diag = torch.full((3, 64), -7.0, dtype=F64, device=device)
    scratch = torch.full((3 * 64 * 64,), 5.0, dtype=F64, device=device)   # room for either kind's ranks
    torch.cuda.synchronize()
    p = dict(panel=_ptr(pan.R), rows=_ptr(rd), tlen=_ptr(td), dg=_ptr(dg), scratch=_ptr(scratch), diag=_ptr(diag),
             out=_ptr(out), status=_ptr(status))
    kw = dict(kw)
    if "null" in kw:
        p[kw.pop("null")] = None
    # the stages of a good call, so that only the argument under test is wrong (Spearman's Gram comes between its two)
    good_stages = _lib.PQ_RANK_RANKS if kind == _lib.PQ_RANK_SPEARMAN else _lib.PQ_RANK_RANKS | _lib.PQ_RANK_FINISH
    rc = _lib.load().pq_rank_cov_batched(
        p["panel"], kw.get("ldp", pan.R.stride(0)), kw.get("n", n), p["rows"], p["tlen"], kw.get("tmax", T), 3, p["dg"],
        kw.get("dg_stride", dg.stride(0)), kw.get("kind", kind), kw.get("mode", _lib.PQ_RANK_COV),
        kw.get("stages", good_stages),
        p["scratch"], n, p["diag"], kw.get("ldd", 64), p["out"], kw.get("ld", 64), kw.get("out_stride", 64 * 64),
        p["status"], engine._stream())
    torch.cuda.synchronize()
    assert rc != 0 and _lib.load().pq_last_error()
    assert torch.all(out == POISON) and torch.all(status == 7) and torch.all(diag == -7) and torch.all(scratch == 5)


def test_spearman_rank_panel_pitch_is_checked(device):
    pan = engine.Panel(_panel()[:, :20])
    rd, td = pan.rows_to_device(*_kernel_rows(17))
    dg = pan.window_sumsq(rd, td, pan.window_means(rd, td))
    out = torch.full((3, 64, 64), POISON, dtype=F64, device=device)
    status = torch.full((3,), 7, dtype=torch.int32, device=device)
    diag = torch.full((3, 64), -7.0, dtype=F64, device=device)
    scratch = torch.full((3 * 64 * 64,), 5.0, dtype=F64, device=device)
    rc = _lib.load().pq_rank_cov_batched(_ptr(pan.R), pan.R.stride(0), 20, _ptr(rd), _ptr(td), 17, 3, _ptr(dg),
                                         dg.stride(0), _lib.PQ_RANK_SPEARMAN, _lib.PQ_RANK_COV, 1, _ptr(scratch), 19,
                                         _ptr(diag), 64, _ptr(out), 64, 64 * 64, _ptr(status), engine._stream())
    torch.cuda.synchronize()
    assert rc != 0 and _lib.load().pq_last_error()
    assert torch.all(status == 7) and torch.all(diag == -7) and torch.all(scratch == 5)
    # a zero batch is no error and launches nothing
    rc = _lib.load().pq_rank_cov_batched(_ptr(pan.R), pan.R.stride(0), 20, _ptr(rd), _ptr(td), 17, 0, _ptr(dg),
                                         dg.stride(0), _lib.PQ_RANK_KENDALL, _lib.PQ_RANK_COV, 3, _ptr(scratch), 20,
                                         _ptr(diag), 64, _ptr(out), 64, 64 * 64, _ptr(status), engine._stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.all(out == POISON) and torch.all(status == 7)


def test_engine_value_errors(device):
    pan = engine.Panel(_panel()[:, :20])
    rd, td = pan.rows_to_device(*_kernel_rows(17))
    out = torch.full((3, 64, 64), POISON, dtype=F64, device=device)
    with pytest.raises(ValueError, match="kind"):
        engine.rank_cov(pan, rd, td, kind="pearson", out=out)
    with pytest.raises(ValueError, match="output"):
        engine.rank_cov(pan, rd, td, output="covariance", out=out)
    with pytest.raises(ValueError, match="out must be"):
        engine.rank_cov(pan, rd, td, out=out[:, :32])
    with pytest.raises(ValueError, match="out must be"):
        engine.rank_cov(pan, rd, td, out=out.to(torch.float32))
    long_rows = torch.zeros((1, _lib.PQ_RANK_TMAX + 1), dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="rows"):
        engine.rank_cov(pan, long_rows, td[:1])
    torch.cuda.synchronize()
    assert torch.all(out == POISON)


# ---- 4. Covariance(method='spearman' / 'kendall') ---------------------------------------------------

def _frame(n, D, seed=None, ties=True):
    dates, R, _, _ = factor_panel(D, n, **({} if seed is None else {"seed": seed}))
    if ties:
        R = _with_ties(R)
    return pd.DataFrame(R, index=pd.DatetimeIndex(dates), columns=[f"A{i:03d}" for i in range(n)])


@pytest.mark.parametrize("kind", KINDS)
def test_covariance_estimate(device, kind):
    X = _frame(12, 60)
    S = Covariance(method=kind, check_positive_definite=False).estimate(X)
    assert isinstance(S, pd.DataFrame) and list(S.index) == list(X.columns) and list(S.columns) == list(X.columns)
    mod = rm.rank_cov(X.to_numpy(), kind)
    worst = float((np.abs(S.to_numpy() - mod.Sigma) / np.outer(mod.sd, mod.sd)).max())
    print(f"Covariance.estimate ({kind}): {worst:.2e}")
    assert worst <= SIGMA_TOL
    assert np.array_equal(COV[kind](X).to_numpy(), S.to_numpy())
    Sn = COV[kind](X.to_numpy())
    assert isinstance(Sn, np.ndarray) and np.array_equal(Sn, S.to_numpy())
    X2 = _frame(40, 30)                                           # more assets than rows
    S2 = Covariance(method=kind, check_positive_definite=True).estimate(X2)
    assert isinstance(S2, pd.DataFrame) and list(S2.columns) == list(X2.columns) and isPD(S2)
    raw = COV[kind](X2)
    if kind == "spearman":                                        # singular: repaired
        assert not np.array_equal(S2.to_numpy(), raw.to_numpy())
    else:                                                         # positive definite as it stands
        assert np.array_equal(S2.to_numpy(), raw.to_numpy())
    Xn = X.copy()
    Xn.iloc[7, 3] = np.nan
    with pytest.raises(ValueError, match="complete windows"):
        Covariance(method=kind).estimate(Xn)
    with pytest.raises(ValueError, match="bad input"):
        Covariance(method=kind).estimate(pd.DataFrame(np.full((10, 6), 0.25)))
    with pytest.raises(ValueError, match="bad input"):
        COV[kind](X.iloc[:1])


@pytest.mark.parametrize("kind", KINDS)
def test_estimate_batch_lr(device, kind):
    T, n = 65, 130
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:-1, :n])
    rd, td = pan.rows_to_device(np.where(rows == 399, 0, rows), lens)
    cov = Covariance(method=kind)
    out = torch.full((3, 192, 192), POISON, dtype=F64, device=device)
    S, pdiag, mu, dg = cov.estimate_batch_lr(pan, rd, td, out=out, materialise=True)
    assert S is out and mu is None and dg is None and torch.equal(pdiag, torch.zeros(3, dtype=F64, device=device))
    ref = engine.rank_cov(pan, rd, td, kind=kind)[0]
    assert torch.equal(S, ref)
    assert not S[:, n:, :].any() and not S[:, :, n:].any()        # the padding of a dense P is zero
    assert torch.equal(cov.estimate_batch(pan, rd, td)[0], ref)
    with pytest.raises(NotImplementedError, match="own window"):
        cov.estimate_batch_lr(pan, rd, td, materialise=False)
    Rn = _panel()[:-1, :n].copy()
    Rn[0, 0] = np.nan
    assert cov.estimate_batch_lr(engine.Panel(Rn), rd, td) == (None, None, None, None)


# ---- 5. MeanVariance: the dense batched route ------------------------------------------------------

def _service(opt, X, rebdates, width, budget=1.0, upper=0.2):
    return BacktestService(
        data={"return_series": X},
        selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
        optimization_item_builders={
            "return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=budget),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, upper=upper)},
        optimization=opt, rebdates=rebdates, quiet=True)


@pytest.mark.parametrize("kind,width,n", [("spearman", 60, 12), ("kendall", 60, 12), ("kendall", 30, 40)])
def test_mean_variance_backtest(device, kind, width, n):
    """The dense batched route: every date against the oracle IPM on P = 2 ra Sigma_model, with the
    bars of tests/test_gerber_gpu.py::test_mean_variance_backtest.  The Kendall case with n = 40 >
    width = 30 is the singular-window case the estimator exists for: its model Sigma is first
    checked on the host to be positive definite."""
    from oracle.qp_ipm import solve_qp
    ra, ndates = 2.0, 6
    X = _frame(n, 100, seed=11)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + ndates]]
    opt = MeanVariance(covariance=Covariance(method=kind), solver_name="mi355x", risk_aversion=ra)
    bt = Backtest()
    bt.run(_service(opt, X, rebdates, width))
    assert bt.stats["solved"] == ndates and bt.stats["path"] == "dense"
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    Xv = X.to_numpy()
    for i, d in enumerate(rebdates):
        e = X.index.get_loc(pd.Timestamp(d))
        Xw = Xv[e - width + 1:e + 1]
        mod = rm.rank_cov(Xw, kind)
        assert mod.status == rm.OK
        if n > width:
            assert np.linalg.eigvalsh(mod.Sigma).min() > 0.0
            np.linalg.cholesky(mod.Sigma)
        P = 2 * ra * mod.Sigma
        q = -rp.mean_geometric(Xw, None, None, None)
        o = solve_qp(P, q, A=np.ones((1, n)), b=np.ones(1), lb=np.zeros(n), ub=np.full(n, 0.2))
        obj = 0.5 * W[i] @ P @ W[i] + q @ W[i]
        assert abs(obj - o.obj) <= 1e-6 * max(abs(o.obj), 1e-12), (i, obj, o.obj)
        assert np.abs(W[i] - o.x).max() < 1e-5, (i, np.abs(W[i] - o.x).max())
        assert abs(W[i].sum() - 1) < 1e-7 and W[i].min() > -1e-7 and W[i].max() < 0.2 + 1e-7


# ---- 6. HierarchicalRiskParity ----------------------------------------------------------------------

SCALE = 0.7


@pytest.mark.parametrize("linkage", ["single", "average"])
@pytest.mark.parametrize("kind", KINDS)
def test_hrp_on_the_rank_matrix(device, kind, linkage):
    """Rank correlations are ratios of small integers and can tie, so the tree is not comparable
    across implementations: the device's own tree is checked for consistency (its leaf order, the
    bisection of that order on the model's Sigma, the multiset of single-linkage merge distances),
    never against another tree; the batched backtest equals the solo solves."""
    n, T, ndates = 24, 100, 6
    X = _frame(n, 140, seed=11)
    rebdates = [str(d.date()) for d in X.index[T + 5:T + 5 + ndates]]

    def make():
        opt = HierarchicalRiskParity(covariance=Covariance(method=kind), linkage=linkage)
        opt.constraints = Constraints(selection=list(X.columns))
        opt.constraints.add_budget(rhs=SCALE)
        return opt
    worst = dict(x=0.0, link=0.0)
    solo = []
    for d in rebdates:
        e = X.index.get_loc(pd.Timestamp(d))
        win = X.iloc[e - T + 1:e + 1]
        opt = make()
        opt.set_objective(OptimizationData(align=False, return_series=win))
        assert opt.solve() is True
        Z = opt.results["linkage"]
        order = np.array([X.columns.get_loc(a) for a in opt.results["order"]])
        assert np.array_equal(order, hm.leaves(Z, n))
        mod = rm.rank_cov(win.to_numpy(), kind)
        assert mod.status == rm.OK
        xm = LD(SCALE) * hm.bisect(mod.Sigma.astype(LD), order)
        x = np.array([opt.results["weights"][a] for a in X.columns])
        worst["x"] = max(worst["x"], float(np.max(np.abs(x - xm) / xm)))
        assert abs(x.sum() - SCALE) <= 1e-14
        if linkage == "single":
            dm = np.sort(hm.prim_edges(hm.distance(mod.Sigma))[2])
            worst["link"] = max(worst["link"], float(np.abs(np.sort(Z[:, 2]) - dm).max()))
        solo.append(x)
    print(f"hrp on {kind} ({linkage}): weights {worst['x']:.2e}, merge distances {worst['link']:.2e}")
    assert worst["x"] <= HRP_TOL and worst["link"] <= LINK_TOL
    bt = Backtest()
    bt.run(_service(make(), X, rebdates, T, budget=SCALE))
    assert bt.stats.get("path") == "hrp"
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    assert W.shape == (ndates, n) and np.array_equal(W, np.stack(solo))


# ---- 7. what the rank covariances do not serve ---------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_risk_parity_needs_a_window_form(device, kind):
    X = _frame(12, 60)
    opt = RiskParity(covariance=Covariance(method=kind))
    opt.constraints = Constraints(selection=list(X.columns))
    opt.set_objective(OptimizationData(align=False, return_series=X))
    with pytest.raises(NotImplementedError):
        opt.solve()
