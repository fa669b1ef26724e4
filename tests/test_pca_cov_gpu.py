"""The PCA factor covariance on the device: pq_window_gram_batched and pq_window_project_batched
against NumPy, engine.pca_window_form against the float64 model (tests/pca_cov_model.py) for both
eigen backends, and the public interface on top of it (Covariance 'pca', RiskParity,
HierarchicalRiskParity, MeanVariance, Backtest).

Every bar below is ten times the worst deviation from the NumPy model seen on MI355X, rounded up
to a power of ten; the deviations are relative to the date's largest variance (Gram diagonal for
the Gram kernel, largest |entry| of the reference rows for the projection).  The observed values
stand beside each bar and in profiles/pca_cov_pytest.txt."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.backtest import Backtest, BacktestService
from porqua_amd.builders import (OptimizationItemBuilder, SelectionItemBuilder, bibfn_box_constraints,
                                 bibfn_budget_constraint, bibfn_return_series, bibfn_selection_data)
from porqua_amd.constraints import Constraints
from porqua_amd.covariance import Covariance, cov_pca
from porqua_amd.optimization import HierarchicalRiskParity, MeanVariance, RiskParity
from porqua_amd.optimization_data import OptimizationData
from porqua_amd.synthetic import factor_panel
from tests import hrp_model as hm
from tests import pca_cov_model as pm
from tests import risk_parity_model as rpm

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
OK, BAD = _lib.PQ_PCA_OK, _lib.PQ_PCA_BAD_INPUT
POISON = 1e150
SHAPES = [(2, 1), (5, 3), (17, 70), (64, 64), (65, 130), (100, 257)]
BACKENDS = ["jacobi", "rocsolver"]

GRAM_TOL = 1e-13       # observed 1.3e-15 (centred and uncentred, every shape)
# the panel with mean 1e3 and spread 1e-2: observed 1.2e-11 centred (1.5e-15 uncentred).  The float64
# window mean of values near 1e3 is rounded at 1e-13, 1e-11 of the spread, and that relative
# error of the centred rows is what remains; centring on the host first would lose as much
GRAM_MEAN_TOL = 1e-9
PROJ_TOL = 1e-14       # observed 8.8e-16
# sigma2, l_j and the dense Sigma of pca_window_form.  Observed, jacobi: sigma2 5.3e-15, l_j 3.6e-13,
# dense 1.7e-14; rocsolver: sigma2 3.7e-16, l_j 1.5e-14, dense 1.7e-15 (the block-Jacobi solver is
# documented at 1.2e-12 on eigenvalues)
FORM_TOL = 1e-11
EST_TOL = 1e-13        # Covariance.estimate: observed 5.6e-15 against sklearn, 8.0e-16 against the model
RP_TOL = 1e-11         # risk-parity weights 3.3e-13 and risk contributions 3.6e-13 (relative; eps = 1e-12)
HRP_TOL = 1e-13        # HRP weights 2.7e-15 (relative)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- panels and row tables (host) ---------------------------------------------------------------

def _kernel_case(T, n, high_mean=False, seed=7):
    """A panel of 2 T + 6 rows, its last row poison, and three windows of up to T rows: consecutive
    rows, every other row, and a shorter window whose unused row slots point at the poison row (a
    valid index: a stray read shows as a wrong number, never as a fault)."""
    rng = np.random.default_rng(seed + 131 * T + n)
    D = 2 * T + 6
    R = 1e3 + 1e-2 * rng.standard_normal((D, n)) if high_mean else rng.normal(3e-4, 0.02, size=(D, n))
    R[-1] = POISON
    short = max(1, T - 3)
    rows = np.full((3, T), D - 1, dtype=np.int32)
    rows[0] = 2 + np.arange(T)
    rows[1] = 1 + 2 * np.arange(T)
    rows[2, :short] = 3 + np.arange(short) + (np.arange(short) > short // 2)
    return R, rows, np.array([T, T, short], dtype=np.int32)


def _centre(R, rows, T, centred=True):
    X = R[rows[:T]].astype(LD)
    return X - X.mean(0) if centred else X


def planted_panel(D, n, nf=3, seed=3):
    """nf strong factors over unit noise (the 'mp' case: the rule has a wide margin at nf)."""
    rng = np.random.default_rng(seed)
    B = rng.normal(0.0, 1.0, size=(n, nf)) * np.array([6.0, 4.5, 3.5][:nf])
    return (rng.standard_normal((D, nf)) @ B.T + rng.standard_normal((D, n))) * 0.01


def windows(D, T, count, step=3):
    rows = np.stack([np.arange(i * step, i * step + T, dtype=np.int32) for i in range(count)])
    assert rows.max() < D
    return rows, np.full(count, T, dtype=np.int32)


FORM_CASES = {"k5": (40, 130, 5), "k3": (60, 24, 3), "mp": (64, 200, "mp")}


def form_case(name):
    T, n, nf = FORM_CASES[name]
    R = planted_panel(T + 12, n) if nf == "mp" else factor_panel(T + 12, n)[1]
    rows, lens = windows(T + 12, T, 4)
    return R, rows, lens, nf


# ---- 1. the Gram kernel ---------------------------------------------------------------------------

def _gram_launch(pan, rd, td, mu, ldg, batch=None, tmax=None, G=None, n=None, null=None):
    B, tm = rd.shape
    batch = B if batch is None else batch
    if G is None:
        G = torch.full((B, ldg, ldg), -7.0, dtype=F64, device=pan.device)
    args = dict(panel=_ptr(pan.R), rows=_ptr(rd), tlen=_ptr(td), G=_ptr(G))
    if null:
        args[null] = None
    rc = _lib.load().pq_window_gram_batched(args["panel"], pan.R.stride(0), pan.n if n is None else n, args["rows"],
                                            args["tlen"], tm if tmax is None else tmax, batch, _ptr(mu),
                                            0 if mu is None else mu.stride(0), args["G"], ldg, ldg * ldg,
                                            engine._stream())
    torch.cuda.synchronize()
    return rc, G


@pytest.mark.parametrize("centred", [True, False])
@pytest.mark.parametrize("T,n", SHAPES)
def test_gram_kernel_matches_numpy(device, T, n, centred):
    worst = {}
    for high_mean in (False, True):
        R, rows, lens = _kernel_case(T, n, high_mean)
        pan = engine.Panel(R)
        rd, td = pan.rows_to_device(rows, lens)
        mu = pan.window_means(rd, td) if centred else None
        ldg = engine.round_up(T, 64) + (64 if T == 64 else 0)
        rc, G = _gram_launch(pan, rd, td, mu, ldg)
        assert rc == 0
        G = G.cpu().numpy()
        err = 0.0
        for b in range(3):
            t = int(lens[b])
            Xc = _centre(R, rows[b], t, centred)
            ref = np.asarray(Xc @ Xc.T, dtype=np.float64)
            # (a centred one-row window: the reference is exactly zero, and so must the kernel be)
            err = max(err, float(np.abs(G[b, :t, :t] - ref).max() / (np.diag(ref).max() or 1.0)))
            assert not G[b, t:, :].any() and not G[b, :, t:].any()             # the padding is exactly zero
            assert np.array_equal(G[b], G[b].T)
        worst[high_mean] = err
    print(f"gram (T, n) = {(T, n)} centred={centred}: {worst[False]:.2e}, mean 1e3: {worst[True]:.2e}")
    assert worst[False] <= GRAM_TOL
    assert worst[True] <= GRAM_MEAN_TOL


# ---- 2. the projection kernel ---------------------------------------------------------------------

def _project_launch(pan, rd, td, mu, V, ldv, col, s, kcnt, kmax, frow, F, ldf, tmax=None, null=None):
    args = dict(panel=_ptr(pan.R), rows=_ptr(rd), tlen=_ptr(td), V=_ptr(V), col=_ptr(col), s=_ptr(s), kcnt=_ptr(kcnt),
                frow=_ptr(frow), F=_ptr(F))
    if null:
        args[null] = None
    rc = _lib.load().pq_window_project_batched(
        args["panel"], pan.R.stride(0), pan.n, args["rows"], args["tlen"], rd.shape[1] if tmax is None else tmax,
        rd.shape[0], _ptr(mu), 0 if mu is None else mu.stride(0), args["V"], ldv, ldv * ldv, args["col"], args["s"],
        args["kcnt"], kmax, args["frow"], args["F"], ldf, engine._stream())
    torch.cuda.synchronize()
    return rc


def _project_case(T, n, k, dev, centred=True):
    """Eigenvectors from NumPy's eigh (the kernel alone is under test), a permuted column table,
    the factor counts (k, 0, about k / 2) and the third date's rows ahead of the first's."""
    R, rows, lens = _kernel_case(T, n)
    rng = np.random.default_rng(5 + T + 7 * k)
    ldv, ldf = T + 3, n + 5
    V = np.zeros((3, ldv, ldv))
    for b in range(3):
        Xc = np.asarray(_centre(R, rows[b], int(lens[b]), centred), dtype=np.float64)
        t = int(lens[b])
        V[b, :t, :t] = np.linalg.eigh(Xc @ Xc.T)[1]
        V[b, t:, :] = POISON                                  # rows past the window are never read
    col = np.stack([rng.integers(0, int(lens[b]), size=k) for b in range(3)]).astype(np.int32)
    s = rng.uniform(0.5, 2.0, size=(3, k))
    kcnt = np.array([k, 0, (k + 1) // 2], dtype=np.int32)
    frow = np.array([kcnt[2], 0, 0], dtype=np.int32)
    return R, rows, lens, V, ldv, ldf, col, s, kcnt, frow


@pytest.mark.parametrize("k", [1, 3, 16, 17, 64])
@pytest.mark.parametrize("T,n", SHAPES)
def test_project_kernel_matches_numpy(device, T, n, k):
    worst = 0.0
    for centred in ((True, False) if (T, n) == (17, 70) else (True,)):
        R, rows, lens, V, ldv, ldf, col, s, kcnt, frow = _project_case(T, n, k, device, centred)
        pan = engine.Panel(R)
        rd, td = pan.rows_to_device(rows, lens)
        mu = pan.window_means(rd, td) if centred else None
        total = int(kcnt.sum())
        F = torch.full((total + 1, ldf), -7.0, dtype=F64, device=device)
        dv = [torch.from_numpy(a).to(device) for a in (V, col, s, kcnt, frow)]
        rc = _project_launch(pan, rd, td, mu, dv[0], ldv, dv[1], dv[2], dv[3], k, dv[4], F, ldf)
        assert rc == 0
        F = F.cpu().numpy()
        assert np.all(F[total] == -7.0)                                        # nothing past the last factor row
        for b in (0, 2):
            t, kc = int(lens[b]), int(kcnt[b])
            Xc = _centre(R, rows[b], t, centred)
            Vk = V[b][:t][:, col[b, :kc]].astype(LD)                           # t x kc: the named columns
            ref = np.asarray(s[b, :kc, None].astype(LD) * (Vk.T @ Xc), dtype=np.float64)
            got = F[frow[b]:frow[b] + kc]
            assert not got[:, n:].any()                                        # the row padding is zero
            worst = max(worst, float(np.abs(got[:, :n] - ref).max() / (np.abs(ref).max() or 1.0)))
    print(f"project (T, n, k) = {(T, n, k)}: {worst:.2e}")
    assert worst <= PROJ_TOL


# ---- 3. / 4. / 6. engine.pca_window_form -----------------------------------------------------------

def _form_host(pf):
    return dict(rows=pf.rows.cpu().numpy(), k=pf.tlen.cpu().numpy(), sigma2=pf.sigma2.cpu().numpy(),
                evals=pf.evals.cpu().numpy(), status=pf.status.cpu().numpy(), F=pf.panel.R.cpu().numpy())


def _dense(h, b, n):
    Z = h["F"][h["rows"][b, :h["k"][b]]]
    return Z.T @ Z + h["sigma2"][b] * np.eye(n)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(FORM_CASES))
def test_window_form_matches_model(device, name, backend):
    R, rows, lens, nf = form_case(name)
    n = R.shape[1]
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    pf = engine.pca_window_form(pan, rd, td, nf, backend=backend)
    h = _form_host(pf)
    assert pf.rows.dtype == torch.int32 and pf.tlen.dtype == torch.int32 and pf.status.dtype == torch.int32
    assert h["rows"].shape == (len(lens), h["k"].max()) and h["evals"].shape == h["rows"].shape
    worst = dict(sigma2=0.0, evals=0.0, dense=0.0)
    for b in range(len(lens)):
        mod = pm.pca_cov(R[rows[b]], nf)
        assert mod.status == pm.OK and h["status"][b] == OK
        if nf == "mp":
            assert mod.k == 3 and mod.margin > 1e-6       # a one-ulp difference cannot change the count
        assert h["k"][b] == mod.k
        top = np.diag(mod.Sigma).max()
        worst["sigma2"] = max(worst["sigma2"], abs(h["sigma2"][b] - mod.sigma2) / top)
        worst["evals"] = max(worst["evals"], np.abs(h["evals"][b, :mod.k] - mod.evals).max() / top)
        assert not h["evals"][b, mod.k:].any()
        worst["dense"] = max(worst["dense"], np.abs(_dense(h, b, n) - mod.Sigma).max() / top)
        assert float((pf.dense(b).cpu() - torch.from_numpy(_dense(h, b, n))).abs().max()) <= 1e-13 * top
    print(f"window form {name} {backend}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= FORM_TOL


def test_window_form_chunks_and_argument_checks(device):
    R, rows, lens, nf = form_case("k5")
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    one = _form_host(engine.pca_window_form(pan, rd, td, nf))
    two = _form_host(engine.pca_window_form(pan, rd, td, nf, chunk_bytes=1))     # one date per chunk
    for key in one:
        assert np.array_equal(one[key], two[key]), key
    n = pan.n
    for bad in (0, n, -1, 2.0, True, "all"):
        with pytest.raises(ValueError, match="n_factors"):
            engine.pca_window_form(pan, rd, td, bad)
    with pytest.raises(ValueError, match="n_factors"):
        engine.pca_window_form(pan, rd, td, 9, kmax=8)
    for kmax in (0, _lib.PQ_PCA_KMAX + 1):
        with pytest.raises(ValueError, match="kmax"):
            engine.pca_window_form(pan, rd, td, "mp", kmax=kmax)
    with pytest.raises(ValueError, match="backend"):
        engine.pca_window_form(pan, rd, td, 3, backend="lapack")
    empty = engine.pca_window_form(pan, rd[:0], td[:0], 3)
    assert empty.rows.shape[0] == 0 and empty.sigma2.shape == (0,) and empty.status.shape == (0,)
    # 'mp' never keeps more than kmax factors
    Rm, rows_m, lens_m, _ = form_case("mp")
    pm_ = engine.Panel(Rm)
    capped = engine.pca_window_form(pm_, *pm_.rows_to_device(rows_m, lens_m), "mp", kmax=2)
    assert torch.all(capped.tlen == 2) and torch.all(capped.status == OK)
    assert pm.pca_cov(Rm[rows_m[0]], "mp", kmax=2).k == 2


def test_identical_launches_are_bitwise_equal(device):
    R, rows, lens = _kernel_case(65, 130)
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    mu = pan.window_means(rd, td)
    G1, G2 = (_gram_launch(pan, rd, td, mu, 128)[1] for _ in range(2))
    assert torch.equal(G1, G2)
    Rf, rows_f, lens_f, nf = form_case("mp")
    pf_ = engine.Panel(Rf)
    rdf, tdf = pf_.rows_to_device(rows_f, lens_f)
    a, b = (_form_host(engine.pca_window_form(pf_, rdf, tdf, nf, backend="jacobi")) for _ in range(2))
    for key in a:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_dates_do_not_affect_their_neighbours(device, backend):
    """A constant window, a window of rank 2 (k = 3 asked) and a one-row window, each between two
    good dates: BAD_INPUT with NaN sigma2 and no factor rows; the good dates' results are those
    of the batch without the bad dates, bit for bit."""
    T, n, k = 60, 24, 3
    R = factor_panel(3 * T + 12, n)[1]
    rng = np.random.default_rng(2)
    R[T + 12:2 * T + 12] = 0.25                                                          # constant rows
    R[2 * T + 12:] = rng.standard_normal((T, 2)) @ rng.standard_normal((2, n)) * 0.01   # rank 2 (centred: <= 2)
    good, lens_g = windows(T + 12, T, 4)
    rows = np.stack([good[0], T + 12 + np.arange(T), good[1], 2 * T + 12 + np.arange(T), good[2],
                     np.r_[5, np.full(T - 1, 0)], good[3]]).astype(np.int32)
    lens = np.array([T, T, T, T, T, 1, T], dtype=np.int32)
    pan = engine.Panel(R)
    mixed = _form_host(engine.pca_window_form(pan, *pan.rows_to_device(rows, lens), k, backend=backend))
    alone = _form_host(engine.pca_window_form(pan, *pan.rows_to_device(good, lens_g), k, backend=backend))
    assert list(mixed["status"]) == [OK, BAD, OK, BAD, OK, BAD, OK] and list(alone["status"]) == [OK] * 4
    for b in (1, 3, 5):
        assert np.isnan(mixed["sigma2"][b]) and mixed["k"][b] == 0 and np.all(np.isnan(mixed["evals"][b]))
        assert pm.pca_cov(R[rows[b, :lens[b]]], k).status == pm.BAD_INPUT
    assert mixed["F"].shape == alone["F"].shape                                          # no factor rows of bad dates
    for g, b in enumerate((0, 2, 4, 6)):
        assert mixed["sigma2"][b] == alone["sigma2"][g] and np.array_equal(mixed["evals"][b], alone["evals"][g])
        assert np.array_equal(mixed["F"][mixed["rows"][b, :k]], alone["F"][alone["rows"][g, :k]])


# ---- 5. host argument checks: an error, nothing launched ------------------------------------------

@pytest.mark.parametrize("kw", [{"ldg": 96}, {"ldg": 64}, {"tmax": _lib.PQ_PCA_TMAX + 1, "ldg": 2048}, {"tmax": 0},
                                {"n": 0}, {"null": "panel"}, {"null": "rows"}, {"null": "tlen"}, {"null": "G"}])
def test_gram_host_argument_checks(device, kw):
    R, rows, lens = _kernel_case(65, 30)
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    kw = dict(kw)
    ldg = kw.pop("ldg", 128)
    G = torch.full((3, 128, 128), -7.0, dtype=F64, device=device)
    rc, _ = _gram_launch(pan, rd, td, None, ldg, G=G, **kw)
    assert rc != 0 and _lib.load().pq_last_error()
    assert torch.all(G == -7.0)


@pytest.mark.parametrize("kw", [{"kmax": 0}, {"kmax": _lib.PQ_PCA_KMAX + 1}, {"ldf": 29}, {"ldv": 64},
                                {"tmax": _lib.PQ_PCA_TMAX + 1}, {"null": "V"}, {"null": "col"}, {"null": "s"},
                                {"null": "kcnt"}, {"null": "frow"}, {"null": "F"}, {"null": "panel"}])
def test_project_host_argument_checks(device, kw):
    T, n, k = 65, 30, 3
    R, rows, lens, V, ldv, ldf, col, s, kcnt, frow = _project_case(T, n, k, device)
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    dv = [torch.from_numpy(a).to(device) for a in (V, col, s, kcnt, frow)]
    F = torch.full((int(kcnt.sum()), ldf), -7.0, dtype=F64, device=device)
    kw = dict(kw)
    rc = _project_launch(pan, rd, td, None, dv[0], kw.pop("ldv", ldv), dv[1], dv[2], dv[3], kw.pop("kmax", k), dv[4], F,
                         kw.pop("ldf", ldf), **kw)
    assert rc != 0 and _lib.load().pq_last_error()
    assert torch.all(F == -7.0)


# ---- 7. Covariance(method='pca') ----------------------------------------------------------------

def _frame(n, D, seed=None):
    dates, R, _, _ = factor_panel(D, n, **({} if seed is None else {"seed": seed}))
    return pd.DataFrame(R, index=pd.DatetimeIndex(dates), columns=[f"A{i:03d}" for i in range(n)])


def test_covariance_estimate(device):
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    X = _frame(24, 60)
    cov = Covariance(method="pca", n_factors=3)
    S = cov.estimate(X)
    assert isinstance(S, pd.DataFrame) and list(S.index) == list(X.columns) and list(S.columns) == list(X.columns)
    ref = PCA(3, svd_solver="full").fit(X.to_numpy()).get_covariance()
    e_sk = float(np.abs(S.to_numpy() - ref).max() / np.diag(ref).max())
    mod = pm.pca_cov(X.to_numpy(), 3)
    assert cov.n_factors_ == 3 and abs(cov.noise_variance_ - mod.sigma2) <= EST_TOL * np.diag(ref).max()
    X2 = _frame(130, 40)
    S2 = cov_pca(X2, 5)
    mod2 = pm.pca_cov(X2.to_numpy(), 5)
    e_mod = float(np.abs(S2.to_numpy() - mod2.Sigma).max() / np.diag(mod2.Sigma).max())
    print(f"Covariance.estimate: vs sklearn {e_sk:.2e}, vs the model {e_mod:.2e}")
    assert e_sk <= EST_TOL and e_mod <= EST_TOL
    assert isinstance(cov_pca(X2.to_numpy(), 5), np.ndarray)
    # the default is the Marchenko-Pastur count
    Rm = form_case("mp")[0][:64]
    cm = Covariance(method="pca")
    Sm = cm.estimate(pd.DataFrame(Rm))
    mm = pm.pca_cov(Rm, "mp")
    assert cm.n_factors_ == mm.k == 3
    assert float(np.abs(Sm.to_numpy() - mm.Sigma).max() / np.diag(mm.Sigma).max()) <= EST_TOL
    Xn = X.copy()
    Xn.iloc[7, 3] = np.nan
    with pytest.raises(ValueError, match="complete windows"):
        cov.estimate(Xn)
    for k in (24, 25):
        with pytest.raises(ValueError, match="n_factors"):
            Covariance(method="pca", n_factors=k).estimate(X)
    with pytest.raises(ValueError, match="bad input"):
        Covariance(method="pca", n_factors=3).estimate(pd.DataFrame(np.full((10, 6), 0.25)))


# ---- 8. RiskParity and HierarchicalRiskParity on the factor form ------------------------------

SCALE = 0.7
WF = {24: 3, 130: 5}     # assets -> factors, T = 60


def _opt_case(n):
    T = 60
    R = factor_panel(T + 12, n)[1]
    rows, lens = windows(T + 12, T, 3, step=5)
    return R, rows, lens, WF[n]


def _with_selection(opt, n):
    opt.constraints = Constraints(selection=[f"A{i}" for i in range(n)])
    opt.constraints.add_budget(rhs=SCALE)
    return opt


@pytest.mark.parametrize("n", list(WF))
def test_risk_parity_on_the_factor_form(device, n):
    R, rows, lens, k = _opt_case(n)
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    cov = Covariance(method="pca", n_factors=k)
    opt = _with_selection(RiskParity(covariance=cov, eps=1e-12, max_sweeps=5000), n)
    x, stats, status, form = opt.solve_windows(pan, rd, td, opt.constraints.selection)
    assert torch.all(status == _lib.PQ_RP_OK)
    assert torch.equal(cov.n_factors_batch_, torch.full((3,), k, dtype=torch.int32, device=device))
    xh = x.cpu().numpy()
    b = rpm.equal_budget(n)
    worst = dict(x=0.0, rc=0.0)
    for d in range(3):
        mod = pm.pca_cov(R[rows[d]], k)
        assert abs(float(cov.noise_variance_batch_[d]) - mod.sigma2) <= FORM_TOL * np.diag(mod.Sigma).max()
        y = rpm.solve(mod.Sigma, b)[0]
        xm = rpm.weights(y, SCALE)
        worst["x"] = max(worst["x"], float(np.max(np.abs(xh[d] - xm) / xm)))
        rc = opt.risk_contributions(pan, rd, td, form, x, d)
        assert abs(rc.sum() - 1.0) <= 1e-14
        rcm = rpm.risk_contributions(mod.Sigma, xm)
        worst["rc"] = max(worst["rc"], float(np.max(np.abs(rc - rcm) / rcm)))
    print(f"risk parity n = {n}: weights {worst['x']:.2e}, risk contributions {worst['rc']:.2e}")
    assert max(worst.values()) <= RP_TOL


@pytest.mark.parametrize("n", list(WF))
def test_hrp_on_the_factor_form(device, n):
    R, rows, lens, k = _opt_case(n)
    pan = engine.Panel(R)
    rd, td = pan.rows_to_device(rows, lens)
    opt = _with_selection(HierarchicalRiskParity(covariance=Covariance(method="pca", n_factors=k)), n)
    x, order, stats, status, Z = opt.solve_windows(pan, rd, td, linkage=True)
    assert torch.all(status == _lib.PQ_HRP_OK)
    # the dense matrix the kernel read: the Gram of the factor rows (the same launch, the same bits)
    pf = engine.pca_window_form(pan, rd, td, k)
    Sd = pf.panel.cov(pf.rows, pf.tlen, mode=1)[:, :n, :n].cpu().numpy()
    c = pf.sigma2.cpu().numpy()
    xh, oh, Zh = x.cpu().numpy(), order.cpu().numpy(), Z.cpu().numpy()
    worst = 0.0
    for d in range(3):
        xd, od, Zd, _ = hm.hrp(hm.sigma(Sd[d], 1.0, c[d]), SCALE)
        assert np.array_equal(oh[d], od)
        assert np.array_equal(Zh[d][:, [0, 1, 3]], np.asarray(Zd[:, [0, 1, 3]], dtype=np.float64))
        mod = pm.pca_cov(R[rows[d]], k)
        top = np.diag(mod.Sigma).max()
        err = float(np.abs(Sd[d] + c[d] * np.eye(n) - mod.Sigma).max() / top)
        xm, om, Zm, st = hm.hrp(mod.Sigma.astype(LD), SCALE)
        # the tree is compared with the model's own where its merge distances are further apart
        # than the measured Sigma error: every date here (the panel's seed was chosen on the CPU)
        assert st[1] > err, "a date whose tree is ambiguous at the Sigma error"
        assert np.array_equal(oh[d], om)
        worst = max(worst, float(np.max(np.abs(xh[d] - xm) / xm)))
    print(f"hrp n = {n}: weights {worst:.2e}")
    assert worst <= HRP_TOL


# ---- 9. Backtest.run ------------------------------------------------------------------------------

def _service(opt, X, rebdates, width, budget=1.0, upper=0.5):
    return BacktestService(
        data={"return_series": X},
        selection_item_builders={"data": SelectionItemBuilder(bibfn=bibfn_selection_data)},
        optimization_item_builders={
            "return_series": OptimizationItemBuilder(bibfn=bibfn_return_series, width=width),
            "budget_constraint": OptimizationItemBuilder(bibfn=bibfn_budget_constraint, budget=budget),
            "box_constraints": OptimizationItemBuilder(bibfn=bibfn_box_constraints, upper=upper)},
        optimization=opt, rebdates=rebdates, quiet=True)


@pytest.mark.parametrize("kind", ["risk_parity", "hrp"])
def test_backtest_batched_equals_serial(device, kind):
    width, n = 60, 24
    X = _frame(n, 100, seed=11)
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + 8]]
    make = {"risk_parity": RiskParity, "hrp": HierarchicalRiskParity}[kind]
    W = []
    for batched in (True, False):
        opt = make(covariance=Covariance(method="pca", n_factors=3))
        bs = _service(opt, X, rebdates, width)
        bs.settings["batched"] = batched
        bt = Backtest()
        bt.run(bs)
        assert bt.stats.get("path") == (kind if batched else None)
        W.append(bt.strategy.get_weights_df().to_numpy(dtype=float))
        assert opt.results["status"] is True
    assert W[0].shape == (8, n) and np.array_equal(W[0], W[1])
    e = X.index.get_loc(pd.Timestamp(rebdates[0]))
    mod = pm.pca_cov(X.to_numpy()[e - width + 1:e + 1], 3)
    if kind == "risk_parity":
        xm = rpm.weights(rpm.solve(mod.Sigma, rpm.equal_budget(n))[0])
    else:
        xm = hm.hrp(mod.Sigma.astype(LD))[0]
    assert float(np.max(np.abs(W[0][0] - xm) / xm)) <= 1e-8      # (the default eps of RiskParity is 1e-10)
    # a window without variance: the date is named
    Xz = X.copy()
    Xz.iloc[:X.index.get_loc(pd.Timestamp(rebdates[2])) + 1] = 0.25
    with pytest.raises(RuntimeError, match=rebdates[0] + ".*bad input"):
        Backtest().run(_service(make(covariance=Covariance(method="pca", n_factors=3)), Xz, rebdates, width))


# ---- 10. MeanVariance ---------------------------------------------------------------------------

def test_mean_variance_takes_the_dense_estimate(device):
    width, n, ra = 60, 24, 2.5
    X = _frame(n, 100, seed=11)
    opt = MeanVariance(covariance=Covariance(method="pca", n_factors=3), solver_name="mi355x", risk_aversion=ra)
    assert opt.objective_batch(None) is None
    win = X.iloc[5:65]
    opt.set_objective(OptimizationData(align=False, return_series=win))
    mod = pm.pca_cov(win.to_numpy(), 3)
    P = opt.objective["P"]
    P = P.to_numpy() if hasattr(P, "to_numpy") else P
    assert float(np.abs(P - 2.0 * ra * mod.Sigma).max() / (2.0 * ra * np.diag(mod.Sigma).max())) <= EST_TOL
    rebdates = [str(d.date()) for d in X.index[width + 5:width + 5 + 4]]
    bs = _service(opt, X, rebdates, width)
    bt = Backtest()
    bt.run(bs)
    assert bt.stats.get("path") is None                        # the serial loop
    W = bt.strategy.get_weights_df().to_numpy(dtype=float)
    assert W.shape == (4, n) and np.abs(W.sum(axis=1) - 1.0).max() <= 1e-8
    ref = MeanVariance(covariance=Covariance(method="pca", n_factors=3), solver_name="mi355x", risk_aversion=ra)
    bs2 = _service(ref, X, rebdates, width)
    for i, d in enumerate(rebdates):
        bs2.prepare_rebalancing(rebalancing_date=d)
        ref.set_objective(optimization_data=bs2.optimization_data)
        ref.model_qpsolvers()
        ref.model.solve()                                       # QuadraticProgram.solve on the dense P
        sol = ref.model["solution"]
        assert sol.found and np.array_equal(W[i], np.asarray(sol.x[:n], dtype=float))
