"""The exponentially weighted covariance on the device: pq_ewma_cov_batched (the weighted-moments
kernel, the direct weighted SYRK and the sliding recursion) against the longdouble model
(tests/ewma_model.py), and the public interface on top of it (engine.ewma_cov, Covariance 'ewma',
MeanVariance on the dense route with the slide plan, HierarchicalRiskParity, RiskParity's refusal).

The age table is built once on the host (engine.ewma_age_weights) and handed to both the device and
the model, so both use the same float64 weights.  The bars are derived below, never fitted; the
observed worst values stand beside each bar and in profiles/ewma_cov_pytest.txt."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.backtest import Backtest, BacktestService
from porqua_amd.builders import (OptimizationItemBuilder, SelectionItemBuilder, bibfn_box_constraints,
                                 bibfn_budget_constraint, bibfn_return_series, bibfn_selection_data)
from porqua_amd.constraints import Constraints
from porqua_amd.covariance import Covariance, cov_ewma
from porqua_amd.optimization import HierarchicalRiskParity, MeanVariance, RiskParity
from porqua_amd.optimization_data import OptimizationData
from porqua_amd.synthetic import factor_panel
from tests import ewma_model as em
from tests import hrp_model as hm

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
INF = float("inf")
OK, BAD = _lib.PQ_EWMA_OK, _lib.PQ_EWMA_BAD_INPUT
POISON = 1e150
CASES = [(2, 1), (5, 3), (15, 70), (16, 64), (17, 70), (63, 64), (65, 130), (252, 130), (300, 20), (1024, 16)]
SPECS = [("halflife", 2.0), ("halflife", 11.2), ("halflife", 63.0), ("halflife", INF), ("decay", 0.94)]

# Sigma relative to sd_i sd_j (the model's weighted standard deviations): the project's bar for a
# two-pass FP64 window second moment (SIGMA_TOL of tests/test_gerber_gpu.py: (T + 4) 2^-53 = 1.2e-13
# at T = 1024, doubled for the two factors, times ten).  By Cauchy-Schwarz every weighted term is
# bounded by sd_i sd_j times the denominator, so a relative error eps per term (the two roundings of
# sqrt(w), the products of table entries in the recursion: at most 32 dates x 1.1e-16) stays eps.
# A float64 simulation of the recursion on the host stays within 5.1e-15.
# Observed: direct kernel 3.3e-15, slide kernel 6.2e-15, diagonal at halflife = inf against np.var
# 5.7e-16, the full matrix at halflife = inf against Panel.cov(mode=0) 0 (the same bits), the
# weighted mean 0.23 of its own bar (_mean_tol)
SIGMA_TOL = 1e-12
HRP_TOL = 1e-13        # HRP weights, relative (the bar of tests/test_gerber_gpu.py).  Observed 1.3e-15


def _mean_tol(T):
    """The weighted mean relative to max |x|: T fused multiply-adds (T 2^-53 of sum |w x| / W1, which
    is at most max |x|), the float64 sum W1 (T 2^-53, relative) and one division."""
    return (2 * T + 2) * 2.0 ** -53


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- fixtures (host) ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _panel():
    R = factor_panel(400, 257, seed=5)[1].copy()
    R[-1] = POISON
    return R


def _kernel_rows(T):
    """Three windows of up to T rows as tests/test_gerber_gpu.py::_kernel_rows builds them --
    consecutive rows, every other row, and a shorter window whose unused slots point at the poison
    row (a valid index: a stray read shows as a wrong number, never as a fault) --, wrapped around
    the panel's 399 data rows where T needs more (a window may hold a row twice)."""
    D = _panel().shape[0]
    m = D - 1
    short = max(2, T - 3)
    rows = np.full((3, T), D - 1, dtype=np.int32)
    rows[0] = (2 + np.arange(T)) % m
    rows[1] = (1 + 2 * np.arange(T)) % m
    rows[2, :short] = (3 + np.arange(short) + (np.arange(short) > short // 2)) % m
    return rows, np.array([T, T, short], dtype=np.int32)


def _kw(spec):
    return {spec[0]: spec[1]}


def _models(R, rows, lens, n, spec):
    """The model of every date of a row table (the table of the batch's tmax, as the device gets it)."""
    wage = engine.ewma_age_weights(rows.shape[1], **_kw(spec))
    return [em.ewma(R[rows[b, :lens[b]], :n], wage) for b in range(rows.shape[0])]


@functools.lru_cache(maxsize=None)
def _kernel_models(T, n, spec):
    rows, lens = _kernel_rows(T)
    return _models(_panel(), rows, lens, n, spec)


def _run(pan, rd, td, spec, plan=None, out="poison"):
    B, n = rd.shape[0], pan.n
    ld = engine.round_up(n, 64)
    if isinstance(out, str):
        out = torch.full((B, ld, ld), POISON, dtype=F64, device=pan.device)
    S, status, mean = engine.ewma_cov(pan, rd, td, plan=plan, out=out, **_kw(spec))
    assert (out is None or S is out) and status.dtype == torch.int32 and mean.dtype == F64
    assert tuple(S.shape) == (B, ld, ld) and tuple(status.shape) == (B,) and tuple(mean.shape) == (B, ld)
    torch.cuda.synchronize()
    return S.cpu().numpy(), status.cpu().numpy(), mean.cpu().numpy()


def _deviation(S, mean, mods, n):
    """Worst |S - model| / (sd_i sd_j) over the good dates, after the exactness checks every date
    has to pass: a symmetric block bit for bit, zero padding, NaN where the model says bad input."""
    worst = 0.0
    for b, mod in enumerate(mods):
        Sb = S[b, :n, :n]
        assert not S[b, n:, :].any() and not S[b, :, n:].any()
        if mod.status != em.OK:
            assert np.isnan(Sb).all()
            continue
        assert np.array_equal(Sb, Sb.T)
        worst = max(worst, float((np.abs(Sb - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
        assert not mean[b, n:].any()
    return worst


# ---- 1. the direct kernel -----------------------------------------------------------------------

@pytest.mark.parametrize("spec", SPECS, ids=lambda s: f"{s[0]}={s[1]}")
@pytest.mark.parametrize("T,n", CASES)
def test_direct_kernel_matches_model(device, T, n, spec):
    rows, lens = _kernel_rows(T)
    R = _panel()
    pan = engine.Panel(R[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    S, st, mean = _run(pan, rd, td, spec)
    mods = _kernel_models(T, n, spec)
    assert list(st) == [OK] * 3 and all(m.status == em.OK for m in mods)
    worst = dict(sigma=_deviation(S, mean, mods, n), mean=0.0, diag=0.0, pearson=0.0)
    for b, mod in enumerate(mods):
        X = R[rows[b, :lens[b]], :n]
        worst["mean"] = max(worst["mean"], float(np.abs(mean[b, :n] - mod.mean).max() / np.abs(X).max())
                            / _mean_tol(lens[b]))
        S1, st1, mean1 = _run(pan, rd[b:b + 1], td[b:b + 1], spec)      # the date alone: the same bits
        assert st1[0] == OK and np.array_equal(S1[0], S[b]) and np.array_equal(mean1[0], mean[b])
        if spec[1] == INF:
            var = X.var(axis=0, ddof=1)
            worst["diag"] = max(worst["diag"], float((np.abs(np.diag(S[b, :n, :n]) - var) / var).max()))
    if spec[1] == INF:   # the ddof = 1 sample covariance: the equal-weight kernel's result
        P = pan.cov(rd, td, mode=0).cpu().numpy()
        for b, mod in enumerate(mods):
            worst["pearson"] = max(worst["pearson"],
                                   float((np.abs(S[b, :n, :n] - P[b, :n, :n]) / np.outer(mod.sd, mod.sd)).max()))
    print(f"ewma direct (T, n) = {(T, n)} {spec[0]} = {spec[1]}: Sigma {worst['sigma']:.2e}, mean "
          f"{worst['mean']:.2f} of its bar, diag {worst['diag']:.2e}, pearson {worst['pearson']:.2e}")
    assert worst["sigma"] <= SIGMA_TOL and worst["diag"] <= SIGMA_TOL and worst["pearson"] <= SIGMA_TOL
    assert worst["mean"] <= 1.0


# ---- 2. the slide kernel ------------------------------------------------------------------------

def _runs(T, s, count, first=5):
    return (first + s * np.arange(count)[:, None] + np.arange(T)[None, :]).astype(np.int32), np.full(count, T, np.int32)


@functools.lru_cache(maxsize=None)
def _slide_case(name):
    """(rows, lens, the expected group starts or None) over the 399 data rows of the panel."""
    D = _panel().shape[0]
    if name == "T17_daily":          # 40 daily dates: a 32-date group and an 8-date group
        return _runs(17, 1, 40) + ([0, 32, 40],)
    if name == "T17_s5":
        return _runs(17, 5, 40) + ([0, 32, 40],)
    if name == "T64_s9":             # crosses the 8-row half-chunk of the [entering; -leaving] operand
        return _runs(64, 9, 36) + ([0, 32, 36],)
    if name == "T64_s21":
        return _runs(64, 21, 16) + ([0, 16],)
    if name == "T252_daily":
        return _runs(252, 1, 33) + ([0, 32, 33],)
    if name == "weekends":           # calendar days with the weekend rows removed (engine.window_rows)
        dates = np.datetime64("2021-01-04") + np.arange(D - 1)
        rows, lens = engine.window_rows(dates, dates[100:140], 30)
        assert lens.min() < lens.max() and lens.max() <= 22          # the lengths change with the weekday
        rows = np.where(np.arange(rows.shape[1])[None, :] < lens[:, None], rows, D - 1).astype(np.int32)
        return rows, lens.astype(np.int32), None
    if name == "shuffled":           # no window is its predecessor's moved by 1..64 rows (T = 70): all anchors
        lo, hi = 5 + 3 * np.arange(10), 200 + 3 * np.arange(10)
        starts = np.stack([hi, lo], axis=1).reshape(-1)
        rows = (starts[:, None] + np.arange(70)[None, :]).astype(np.int32)
        return rows, np.full(20, 70, np.int32), list(range(21))
    if name == "mixed":              # window lengths change inside the table: the groups break there
        lens = np.array([17] * 10 + [20] * 10 + [12] + [20] * 5 + [17] * 4, dtype=np.int32)
        rows = np.full((len(lens), 20), D - 1, dtype=np.int32)
        for b, L in enumerate(lens):
            rows[b, :L] = 30 + b + np.arange(L) + (20 - L)           # every window ends one row later
        return rows, lens, [0, 10, 20, 21, 26, 30]
    raise KeyError(name)


SLIDE_CASES = ["T17_daily", "T17_s5", "T64_s9", "T64_s21", "T252_daily", "weekends", "shuffled", "mixed"]
SLIDE_SPECS = [("halflife", 2.0), ("halflife", 11.2), ("halflife", INF)]


@functools.lru_cache(maxsize=None)
def _slide_models(name, n, spec):
    rows, lens, _ = _slide_case(name)
    return _models(_panel(), rows, lens, n, spec)


@pytest.mark.parametrize("spec", SLIDE_SPECS, ids=lambda s: f"{s[0]}={s[1]}")
@pytest.mark.parametrize("n", [130, 70])
@pytest.mark.parametrize("name", SLIDE_CASES)
def test_slide_kernel_matches_model(device, name, n, spec):
    rows, lens, groups = _slide_case(name)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    plan = engine.SlidePlan(rows, lens, pan.device)
    if groups is not None:
        assert plan.gstart.cpu().tolist() == groups
    mods = _slide_models(name, n, spec)
    assert all(m.status == em.OK for m in mods)
    Sp, stp, mp = _run(pan, rd, td, spec, plan=plan)
    Sd, std, md = _run(pan, rd, td, spec)
    assert not stp.any() and not std.any() and np.array_equal(mp, md)
    wp, wd = _deviation(Sp, mp, mods, n), _deviation(Sd, md, mods, n)
    anchors = plan.gstart.cpu().numpy()[:-1]
    assert np.array_equal(Sp[anchors], Sd[anchors])                   # an anchor is the direct kernel's date
    print(f"ewma slide {name} n = {n} {spec[0]} = {spec[1]}: plan {wp:.2e}, direct {wd:.2e} "
          f"({plan.ngroups} groups of {len(lens)} dates)")
    assert wp <= SIGMA_TOL and wd <= SIGMA_TOL


# ---- 3. exactness and edges ---------------------------------------------------------------------

def test_batch_splits_and_repeats_are_bitwise_equal(device):
    n, spec = 130, ("halflife", 11.2)
    rows, lens, _ = _slide_case("T17_daily")
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    whole = _run(pan, rd, td, spec)
    for k in (1, 13, 39):
        a, b = _run(pan, rd[:k], td[:k], spec), _run(pan, rd[k:], td[k:], spec)
        for w, x, y in zip(whole, a, b):
            assert np.array_equal(w, np.concatenate([x, y]))
    plan = engine.SlidePlan(rows, lens, pan.device)
    slide = _run(pan, rd, td, spec, plan=plan)
    again = _run(pan, rd, td, spec, plan=plan)
    a = _run(pan, rd[:32], td[:32], spec, plan=engine.SlidePlan(rows[:32], lens[:32], pan.device))
    b = _run(pan, rd[32:], td[32:], spec, plan=engine.SlidePlan(rows[32:], lens[32:], pan.device))
    for w, r, x, y in zip(slide, again, a, b):                        # split between two slide groups
        assert np.array_equal(w, r) and np.array_equal(w, np.concatenate([x, y]))
    # an out that was not passed is allocated, with zero padding
    S, st, mean = _run(pan, rd, td, spec, out=None)
    assert np.array_equal(S, whole[0]) and not S[:, n:, :].any() and not S[:, :, n:].any()
    empty = engine.ewma_cov(pan, rd[:0], td[:0])
    assert empty[0].shape == (0, 192, 192) and empty[1].shape == (0,) and empty[2].shape == (0, 192)


def _expect_split(pan, rows, lens, spec, bad, with_plan):
    """The batch with its bad dates cut out: the dates before and after them, each part run on its
    own (with its own slide plan), and the NaN blocks."""
    parts, lo = [], 0
    B, ld = rows.shape[0], engine.round_up(pan.n, 64)
    for b in sorted(bad) + [B]:
        if b > lo:
            r, t = pan.rows_to_device(rows[lo:b], lens[lo:b])
            plan = engine.SlidePlan(rows[lo:b], lens[lo:b], pan.device) if with_plan else None
            S, st, _ = _run(pan, r, t, spec, plan=plan)
            assert not st.any()
            parts.append(S)
        if b < B:
            blk = np.zeros((1, ld, ld))
            blk[0, :pan.n, :pan.n] = np.nan
            parts.append(blk)
        lo = b + 1
    return np.concatenate(parts)


@pytest.mark.parametrize("value", [INF, -INF, float("nan")])
def test_bad_value_inside_a_slide_group(device, value):
    """A non-finite value in the row that enters the window of date 8 (T = 17, s = 5) stays for the
    dates 8..11 of a 20-date slide group: they are BAD_INPUT with a NaN block; the dates before
    them carry the bits of the run that ends at date 7, the dates after them the bits of the run
    that starts at date 12 (the recursion starts afresh there), and all meet the bar."""
    n, spec = 70, ("halflife", 11.2)
    rows, lens = _runs(17, 5, 20)
    R = _panel()[:, :n].copy()
    R[rows[8, -1], 3] = value
    bad = [8, 9, 10, 11]
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    mods = _models(R, rows, lens, n, spec)
    assert [b for b, m in enumerate(mods) if m.status != em.OK] == bad
    for with_plan in (True, False):
        plan = engine.SlidePlan(rows, lens, pan.device) if with_plan else None
        assert plan is None or plan.ngroups == 1
        S, st, mean = _run(pan, rd, td, spec, plan=plan)
        assert list(st) == [BAD if b in bad else OK for b in range(20)]
        assert _deviation(S, mean, mods, n) <= SIGMA_TOL
        assert np.array_equal(S, _expect_split(pan, rows, lens, spec, bad, with_plan), equal_nan=True)


def test_one_row_window_and_fast_decay(device):
    n, spec = 70, ("halflife", 2.0)
    rows, lens, _ = _slide_case("T17_daily")
    rows, lens = rows[:12].copy(), lens[:12].copy()
    lens[5] = 1
    rows[5, 1:] = _panel().shape[0] - 1
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    mods = _models(_panel(), rows, lens, n, spec)
    for with_plan in (True, False):
        plan = engine.SlidePlan(rows, lens, pan.device) if with_plan else None
        S, st, mean = _run(pan, rd, td, spec, plan=plan)
        assert list(st) == [OK] * 5 + [BAD] + [OK] * 6
        assert _deviation(S, mean, mods, n) <= SIGMA_TOL
        assert np.array_equal(S, _expect_split(pan, rows, lens, spec, [5], with_plan), equal_nan=True)
    # a half-life of 0.01 rows: W1 = W2 = 1 in float64, the denominator is 0 and every date is bad input
    rows, lens, _ = _slide_case("T17_daily")
    rd, td = pan.rows_to_device(rows, lens)
    for plan in (None, engine.SlidePlan(rows, lens, pan.device)):
        S, st, _ = _run(pan, rd, td, ("halflife", 0.01), plan=plan)
        assert list(st) == [BAD] * 40 and np.isnan(S[:, :n, :n]).all()
        assert not S[:, n:, :].any() and not S[:, :, n:].any()


@pytest.mark.parametrize("kw", [{"tmax": _lib.PQ_EWMA_TMAX + 1}, {"tmax": 0}, {"n": 0}, {"ld": 19}, {"ld": 128, "os": 64},
                                {"ms": 32}, {"null": "panel"}, {"null": "rows"}, {"null": "tlen"}, {"null": "wage"},
                                {"null": "wsqrt"}, {"null": "mean"}, {"null": "wsum"}, {"null": "out"}, {"null": "status"},
                                {"null": "shift"}])
def test_host_argument_checks(device, kw):
    T, n = 17, 20
    rows, lens = _kernel_rows(T)
    pan = engine.Panel(_panel()[:, :n])
    rd, td = pan.rows_to_device(rows, lens)
    plan = engine.SlidePlan(rows, lens, device)
    out = torch.full((3, 64, 64), POISON, dtype=F64, device=device)
    status = torch.full((3,), 7, dtype=torch.int32, device=device)
    mean = torch.full((3, 64), POISON, dtype=F64, device=device)
    wsum = torch.full((3, 2), POISON, dtype=F64, device=device)
    wage = torch.from_numpy(engine.ewma_age_weights(T, halflife=5)).to(device)
    wsqrt = torch.full((T + 1,), POISON, dtype=F64, device=device)
    torch.cuda.synchronize()
    p = dict(panel=_ptr(pan.R), rows=_ptr(rd), tlen=_ptr(td), wage=_ptr(wage), wsqrt=_ptr(wsqrt), mean=_ptr(mean),
             wsum=_ptr(wsum),
             out=_ptr(out), status=_ptr(status), gstart=_ptr(plan.gstart), shift=_ptr(plan.shift))
    kw = dict(kw)
    if "null" in kw:
        p[kw.pop("null")] = None
    ld = kw.get("ld", 64)
    rc = _lib.load().pq_ewma_cov_batched(
        p["panel"], pan.R.stride(0), kw.get("n", n), p["rows"], p["tlen"], kw.get("tmax", T), 3, p["wage"], p["wsqrt"],
        p["mean"],
        kw.get("ms", 64), p["wsum"], p["out"], ld, kw.get("os", 64 * 64), p["status"], p["gstart"], plan.ngroups,
        p["shift"], engine._stream())
    torch.cuda.synchronize()
    assert rc != 0 and _lib.load().pq_last_error()
    assert torch.all(out == POISON) and torch.all(status == 7) and torch.all(mean == POISON) and torch.all(wsum == POISON)
    assert torch.all(wsqrt == POISON)


def test_engine_argument_checks(device):
    rows, lens = _kernel_rows(17)
    pan = engine.Panel(_panel()[:, :20])
    rd, td = pan.rows_to_device(rows, lens)
    out = torch.full((3, 64, 64), POISON, dtype=F64, device=device)
    for bad in ({"halflife": 5, "decay": 0.9}, {"decay": 0}, {"decay": 1.5}, {"halflife": 0}, {"halflife": -1},
                {"halflife": True}):
        with pytest.raises(ValueError, match="ewma"):
            engine.ewma_cov(pan, rd, td, out=out, **bad)
    with pytest.raises(ValueError, match="out must be"):
        engine.ewma_cov(pan, rd, td, out=out[:, :32])
    with pytest.raises(ValueError, match="out must be"):
        engine.ewma_cov(pan, rd, td, out=out.to(torch.float32))
    wide = torch.zeros((1, _lib.PQ_EWMA_TMAX + 1), dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="supported"):
        engine.ewma_cov(pan, wide, td[:1])
    torch.cuda.synchronize()
    assert torch.all(out == POISON)


# ---- 4. Covariance(method='ewma') ---------------------------------------------------------------

def _frame(n, D, seed=None):
    dates, R, _, _ = factor_panel(D, n, **({} if seed is None else {"seed": seed}))
    return pd.DataFrame(R, index=pd.DatetimeIndex(dates), columns=[f"A{i:03d}" for i in range(n)])


def test_covariance_estimate(device):
    X = _frame(12, 60)
    worst = 0.0
    for kw in ({}, {"halflife": 11.2}, {"decay": 0.97}, {"halflife": INF}):
        S = Covariance(method="ewma", check_positive_definite=False, **kw).estimate(X)
        assert isinstance(S, pd.DataFrame) and list(S.index) == list(X.columns) and list(S.columns) == list(X.columns)
        mod = em.ewma(X.to_numpy(), engine.ewma_age_weights(60, **kw))
        worst = max(worst, float((np.abs(S.to_numpy() - mod.Sigma) / np.outer(mod.sd, mod.sd)).max()))
        assert np.array_equal(cov_ewma(X, **kw).to_numpy(), S.to_numpy())
    print(f"Covariance.estimate: {worst:.2e}")
    assert worst <= SIGMA_TOL
    assert isinstance(cov_ewma(X.to_numpy()), np.ndarray)
    ref = np.cov(X.to_numpy(), rowvar=False, aweights=0.94 ** np.arange(59, -1, -1.0))
    assert np.abs(cov_ewma(X.to_numpy()) - ref).max() <= SIGMA_TOL * np.diag(ref).max()
    Xn = X.copy()
    Xn.iloc[7, 3] = np.nan
    with pytest.raises(ValueError, match="complete windows"):
        Covariance(method="ewma").estimate(Xn)
    with pytest.raises(ValueError, match="bad input"):
        Covariance(method="ewma", halflife=0.01).estimate(X)
    with pytest.raises(ValueError, match="bad input"):
        cov_ewma(X.iloc[:1])


def test_estimate_batch_lr(device):
    n = 130
    rows, lens, _ = _slide_case("T17_daily")
    pan = engine.Panel(_panel()[:-1, :n])
    rd, td = pan.rows_to_device(rows, lens)
    plan = engine.SlidePlan(rows, lens, device)
    cov = Covariance(method="ewma", halflife=11.2)
    out = torch.full((40, 192, 192), POISON, dtype=F64, device=device)
    S, pdiag, mu, dg = cov.estimate_batch_lr(pan, rd, td, out=out, plan=plan, materialise=True)
    assert S is out and mu is None and dg is None and torch.equal(pdiag, torch.zeros(40, dtype=F64, device=device))
    assert torch.equal(S, engine.ewma_cov(pan, rd, td, halflife=11.2, plan=plan)[0])   # the slide kernel
    direct = engine.ewma_cov(pan, rd, td, halflife=11.2)[0]
    assert torch.equal(cov.estimate_batch(pan, rd, td)[0], direct)
    assert not torch.equal(S, direct)                                 # (the recursion rounds differently)
    with pytest.raises(NotImplementedError, match="differs from date to date"):
        cov.estimate_batch_lr(pan, rd, td, materialise=False)
    Rn = _panel()[:-1, :n].copy()                                     # missing values: not batched
    Rn[7, 3] = np.nan
    assert cov.estimate_batch_lr(engine.Panel(Rn), rd, td, plan=plan) == (None, None, None, None)


# ---- 5. MeanVariance: the dense batched route with the slide plan ----------------------------------

def _service(opt, X, rebdates, width, budget=1.0, upper=0.2, **settings):
    return BacktestService(
        data={"return_series": X},
        selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
        optimization_item_builders={
            "return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=budget),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, upper=upper)},
        optimization=opt, rebdates=rebdates, quiet=True, **settings)


def test_mean_variance_backtest(device, monkeypatch):
    """12 daily dates with T = 40: the batched dense route hands the stage's slide plan to
    engine.ewma_cov (recorded here, not assumed), and its weights agree with the serial
    set_objective / solve loop to the bar tests/test_gerber_gpu.py::test_mean_variance_backtest
    sets for weights (1e-5).  24 assets, fewer than the window has rows: the serial loop repairs a
    singular estimate with nearestPD, the batched route does not, so only a definite estimate gives
    both loops the same problem."""
    width, n, ra, ndates = 40, 24, 2.0, 12
    X = _frame(n, 100, seed=11)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + ndates]]
    calls = []
    real = engine.ewma_cov

    def spy(panel, rows, tlen, halflife=None, decay=None, plan=None, out=None):
        calls.append((int(rows.shape[0]), plan))
        return real(panel, rows, tlen, halflife=halflife, decay=decay, plan=plan, out=out)
    monkeypatch.setattr(engine, "ewma_cov", spy)

    def make():
        return MeanVariance(covariance=Covariance(method="ewma", halflife=11.2), solver_name="mi355x", risk_aversion=ra)
    bt = Backtest()
    bt.run(_service(make(), X, rebdates, width))
    assert bt.stats["solved"] == ndates and bt.stats["path"] == "dense"
    assert len(calls) == 1 and calls[0][0] == ndates
    plan = calls[0][1]
    assert isinstance(plan, engine.SlidePlan) and plan.ngroups == 1 and plan.shift.cpu().tolist() == [0] + [1] * 11
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    calls.clear()
    bs = Backtest()
    bs.run(_service(make(), X, rebdates, width, batched=False))
    assert bs.stats.get("path") is None                               # the serial loop
    assert len(calls) == ndates and all(c == (1, None) for c in calls)
    Ws = bs.strategy.get_weights_df().to_numpy(dtype=float)
    assert W.shape == Ws.shape == (ndates, n)
    print(f"MeanVariance 'ewma': batched (slide) against serial weights {np.abs(W - Ws).max():.2e}")
    assert np.abs(W - Ws).max() < 1e-5
    assert np.abs(W.sum(axis=1) - 1).max() < 1e-7 and W.min() > -1e-7 and W.max() < 0.2 + 1e-7
    # the objective is the model's: P = 2 ra Sigma_model on the first date
    e = X.index.get_loc(pd.Timestamp(rebdates[0]))
    mod = em.ewma(X.to_numpy()[e - width + 1:e + 1], engine.ewma_age_weights(width, halflife=11.2))
    opt = make()
    opt.covariance.spec["check_positive_definite"] = False
    opt.set_objective(OptimizationData(align=False, return_series=X.iloc[e - width + 1:e + 1]))
    P = np.asarray(opt.objective["P"], dtype=float)
    assert float((np.abs(P - 2 * ra * mod.Sigma) / (2 * ra * np.outer(mod.sd, mod.sd))).max()) <= SIGMA_TOL


# ---- 6. HierarchicalRiskParity and RiskParity ----------------------------------------------------------

SCALE = 0.7


def test_hrp_on_the_ewma_matrix(device):
    """Single-linkage HRP on the dense 'ewma' estimate against tests/hrp_model.py run on the model's
    matrices: the same leaf order (the merge distances of continuous data do not tie: the smallest
    gap is asserted) and the weights at HRP_TOL; the batched backtest equals the solo solves."""
    n, T, ndates = 24, 100, 6
    X = _frame(n, 140, seed=11)
    rebdates = [str(d.date()) for d in X.index[T + 5:T + 5 + ndates]]
    wage = engine.ewma_age_weights(T, halflife=21)

    def make():
        opt = HierarchicalRiskParity(covariance=Covariance(method="ewma", halflife=21))
        opt.constraints = Constraints(selection=list(X.columns))
        opt.constraints.add_budget(rhs=SCALE)
        return opt
    worst, solo = 0.0, []
    for d in rebdates:
        e = X.index.get_loc(pd.Timestamp(d))
        win = X.iloc[e - T + 1:e + 1]
        opt = make()
        opt.set_objective(OptimizationData(align=False, return_series=win))
        assert opt.solve() is True
        xm, order, Z, stats = hm.hrp(em.ewma(win.to_numpy(), wage).Sigma, SCALE)
        assert stats[1] >= 1e-9
        assert [X.columns.get_loc(a) for a in opt.results["order"]] == list(order)
        x = np.array([opt.results["weights"][a] for a in X.columns])
        worst = max(worst, float(np.max(np.abs(x - xm) / xm)))
        assert abs(x.sum() - SCALE) <= 1e-14
        solo.append(x)
    print(f"hrp on ewma: weights {worst:.2e}")
    assert worst <= HRP_TOL
    bt = Backtest()
    bt.run(_service(make(), X, rebdates, T, budget=SCALE))
    assert bt.stats.get("path") == "hrp"
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    assert W.shape == (ndates, n) and np.array_equal(W, np.stack(solo))


def test_risk_parity_needs_a_window_form(device):
    X = _frame(12, 60)
    opt = RiskParity(covariance=Covariance(method="ewma"))
    opt.constraints = Constraints(selection=list(X.columns))
    opt.set_objective(OptimizationData(align=False, return_series=X))
    with pytest.raises(NotImplementedError, match="ewma.*weight"):
        opt.solve()
