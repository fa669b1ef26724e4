"""tests/window_model.py on the CPU: the longdouble model against numpy and pandas on the inputs
of the GPU test, the planner features those inputs are there for, and float64 restatements of the
four sliding algorithms against the model under the sliding bars -- on the exact plans and
panels tests/test_window_kernels_gpu.py uses, so the bars are shown to be reachable by a correct
float64 implementation before a GPU is involved."""
import numpy as np
import pandas as pd
import pytest

from oracle import ref_pipeline as rp
from tests import window_model as wm

LD = wm.LD


def _close(a, b, tol):
    return wm.fro_rel(a, b) <= tol


@pytest.mark.parametrize("offset", wm.OFFSETS)
@pytest.mark.parametrize("tmax", wm.TMAXES)
def test_model_matches_numpy_and_pandas(tmax, offset):
    n = 65
    R, y = wm.base_panel(n, offset)
    Rn = wm.nan_panel(n, offset)
    rows, tlen = wm.row_table(tmax)
    assert rows.min() == 0 and (rows[np.arange(tmax)[None, :] < tlen[:, None]] >= wm.BASE).all()
    for d in range(6):
        rr = rows[d, :tlen[d]]
        X, yw, Xn = R[rr], y[rr], Rn[rr]
        df = pd.DataFrame(X)
        assert _close(wm.mean(X), df.mean().values, 1e-14)
        assert _close(wm.geomean(X), np.exp(np.log(1 + X).mean(0)) - 1, 1e-11)
        assert _close(wm.geomean(X), (1.0 + X).prod(0) ** (1.0 / len(X)) - 1.0, 1e-11)
        assert _close(wm.sumsq(X, False), (X * X).sum(0), 1e-14)
        assert _close(wm.gram(X), X.T @ X, 1e-14)
        assert _close(wm.xty(X, yw), X.T @ yw, 1e-13)
        assert abs(wm.yty(yw) - yw @ yw) <= 1e-14 * float(yw @ yw)
        if tlen[d] > 1:
            assert _close(wm.sumsq(X), ((X - X.mean(0)) ** 2).sum(0), 1e-11)
            assert _close(wm.cov(X), np.cov(X, rowvar=False).reshape(n, n), 1e-12)
            assert _close(wm.cov(X), df.cov().values, 1e-12)
            assert _close(wm.cov(X), rp.cov_pearson(X), 1e-12)
        # skipna forms: the NaN pattern and the values of pandas
        dn = pd.DataFrame(Xn)
        for geometric, ref in ((False, dn.mean().values),
                               (True, np.expm1(np.log1p(dn).mean().values))):
            m = wm.nanmean(Xn, geometric).astype(np.float64)
            assert np.array_equal(np.isnan(m), np.isnan(ref)) and np.isnan(m[2])
            ok = ~np.isnan(ref)
            assert _close(m[ok], ref[ok], 1e-11)
    # the NaN panel has what it promises inside the full window
    Xn = Rn[rows[0, :tlen[0]]]
    ok = ~np.isnan(Xn)
    assert not ok[:, 2].any() and (ok[:, 3] & ok[:, 4]).sum() == (1 if tmax >= 2 else 0)
    assert np.isnan(rp.cov_pairwise(Xn)[3, 4])


def test_minus_100_percent_in_the_model():
    """log1p(-1) = -inf gives exactly -1, a return below -1 gives NaN, in the per-window model."""
    X = np.array([[0.01, -1.0, -1.5, np.nan], [0.02, 0.03, 0.01, -1.0]])
    g = wm.geomean(X[:, :3]).astype(np.float64)
    assert g[1] == -1.0 and np.isnan(g[2]) and abs(g[0] - (np.sqrt(1.01 * 1.02) - 1)) < 1e-15
    assert wm.nanmean(X, geometric=True).astype(np.float64)[3] == -1.0


@pytest.mark.parametrize("cal,T", wm.GROUP_CASES)
def test_plans_have_their_features(cal, T):
    wm.check_features(wm.plan(cal, T))


def test_width_two_on_weekend_rows_cannot_be_grouped():
    """On a calendar that keeps its weekend rows a width of 2 leaves windows of 0 and 1 weekday
    rows: GroupPlan declines them (ok False), so the grouped passes never see that plan and
    T = 2 is exercised on the weekday calendar."""
    p = wm.Plan("weekend", 2)
    assert p.tlen.min() < 2 and not p.gp.ok


def _worst(name, got, model, N, S):
    r = wm.units(got, model, S)
    w = float((r / N.reshape((-1,) + (1,) * (r.ndim - 1))).max())
    print(f"[window-model] {name}: max |f64 - model| / (u S) = {float(r.max()):.2f}, of the bar {w:.3f}")
    return w


@pytest.mark.parametrize("offset", wm.OFFSETS)
@pytest.mark.parametrize("n", wm.NS)
@pytest.mark.parametrize("cal,T", wm.GROUP_CASES)
def test_grouped_restatements_meet_the_sliding_bars(cal, T, n, offset):
    p = wm.plan(cal, T)
    R, y = wm.base_panel(n, offset)
    tag = f"{cal} T={T} n={n} +{offset:g}"
    mu_m = np.stack([wm.mean(R[p.window(b)]) for b in range(p.B)])
    dg_m = np.stack([wm.sumsq(R[p.window(b)]) for b in range(p.B)])
    mu, dg = wm.moments_grp_f64(R, p)
    N, Sm, Sd = wm.moments_bars(R, p, mu_m)
    assert _worst(f"moments mu {tag}", mu, mu_m, N, Sm) <= 1.0
    assert _worst(f"moments dg {tag}", dg, dg_m, N, Sd) <= 1.0
    sxy, dq, yy = wm.gram_xy_grp_f64(R, y, p)
    N, Sx, Sq, Ny, Sy = wm.gram_xy_bars(R, y, p)
    assert _worst(f"gram_xy X'y {tag}", sxy, np.stack([wm.xty(R[p.window(b)], y[p.window(b)]) for b in range(p.B)]), N, Sx) <= 1.0
    assert _worst(f"gram_xy dg {tag}", dq, np.stack([wm.sumsq(R[p.window(b)], False) for b in range(p.B)]), N, Sq) <= 1.0
    assert _worst(f"gram_xy y'y {tag}", yy, np.array([wm.yty(y[p.window(b)]) for b in range(p.B)]), Ny, Sy) <= 1.0
    ge_m = np.stack([wm.geomean(R[p.window(b)]) for b in range(p.B)])
    N, Sg = wm.geomean_bars(R, p, ge_m)
    assert _worst(f"geomean {tag}", wm.geomean_grp_f64(R, p), ge_m, N, Sg) <= 1.0


@pytest.mark.parametrize("offset", wm.OFFSETS)
@pytest.mark.parametrize("n", wm.NS)
@pytest.mark.parametrize("cal,T", wm.SLIDE_CASES)
def test_slide_restatement_meets_the_sliding_bar(cal, T, n, offset):
    p = wm.plan(cal, T)
    R = wm.base_panel(n, offset)[0]
    for mode in (0, 1):
        m, model, N, S = wm.slide_model(cal, T, n, offset, mode)
        got = wm.syrk_slide_f64(R, m, p, mode)
        assert _worst(f"slide mode {mode} {cal} T={T} n={n} +{offset:g}", got, model, N, S) <= 1.0
        if mode == 0:   # the function of (X, m) the kernel evaluates is np.cov to the per-date bar
            for d in range(p.B):
                assert wm.fro_rel(model[d], wm.cov(R[p.window(d)])) <= 1e-12


@pytest.mark.parametrize("T", [5, 30])
def test_geomean_restatement_with_minus_100_percent(T):
    """The sliding log sum with the two counts gives -1 / NaN in exactly the windows that hold
    the planted rows and meets the bar in every other window and column."""
    R, c1, r1, c2, r2 = wm.minus100_case(T)
    p = wm.plan("weekday", T)
    model = np.stack([wm.geomean(R[p.window(b)]) for b in range(p.B)])
    has1 = np.array([r1 in p.window(b) for b in range(p.B)])
    has2 = np.array([r2 in p.window(b) for b in range(p.B)])
    # each planted row enters and leaves inside one group
    for has in (has1, has2):
        hit = np.flatnonzero(has)
        g = np.searchsorted(p.gdates, hit[0], side="right") - 1
        assert len(hit) and p.gdates[g] < hit[0] and hit[-1] < p.gdates[g + 1] - 1
    mf = model.astype(np.float64)
    assert np.array_equal(mf[:, c1] == -1.0, has1) and np.array_equal(np.isnan(mf[:, c2]), has2)
    got = wm.geomean_grp_f64(R, p)
    assert np.array_equal(got[:, c1] == -1.0, has1) and np.array_equal(np.isnan(got[:, c2]), has2)
    assert np.isnan(got).sum() == has2.sum()
    N, S = wm.geomean_bars(R, p, model)
    fin = np.isfinite(mf) & (mf != -1.0)
    r = np.where(fin, wm.units(np.where(fin, got, 0.0), np.where(fin, model, 0.0), S), 0.0)
    assert (r / N[:, None]).max() <= 1.0
