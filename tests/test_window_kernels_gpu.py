"""The eleven window-statistics kernels of porqua_amd/csrc/cov.hip (K1) against the longdouble
model of tests/window_model.py, through the C API, on the windows the planners emit: ragged and
weekend-gapped row tables, windows shorter than an MFMA chunk, n across the 256-column block,
slide plans and group plans of window_rows / slide_plan / GroupPlan on a calendar with weekend
rows and on a weekday calendar whose shifts cross the slide chunk of 8 and the window length.

Every panel has a row pitch of n + 3; row 0 (the padding index of the row tables) and the three
pitch columns hold a poison value (NaN; 1e300 for the NaN-aware kernels), so a stray read is a
wrong number, never a fault.  Output buffers are pre-filled: what a kernel must not write keeps
its fill.  Bars: window_model's docstring."""
import numpy as np
import pytest
import torch

from oracle import ref_pipeline as rp
from porqua_amd import _lib
from tests import window_model as wm

pytestmark = pytest.mark.gpu

F64 = torch.float64
FILL = -7.0
WORST = {}      # kernel -> largest |kernel - model| / (u S) seen, and the largest fraction of N u S


def _ld_of(n):
    return (n + 63) // 64 * 64


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _full(shape, value, device):
    return torch.full(shape, value, dtype=F64, device=device)


def _ok(rc, lib):
    assert rc == 0, lib.pq_last_error()


class _Panel:
    """A poisoned, pitched panel (and benchmark) on the device."""

    def __init__(self, R, device, poison, y=None):
        self.n = R.shape[1]
        self.P = _dev(wm.pitched(R, poison), device)
        self.ptr, self.ldp = self.P.data_ptr(), self.P.stride(0)
        assert self.ldp == self.n + 3
        if y is not None:
            yp = np.array(y)
            yp[0] = poison
            self.y = _dev(yp, device)


def _note(kernel, case, got, model, N, S):
    """Assert |got - model| <= N u S elementwise; record and print the observed units."""
    r = wm.units(got, model, S)
    frac = r / np.asarray(N).reshape((-1,) + (1,) * (r.ndim - 1))
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], float(r.max())), max(w[1], float(frac.max()))
    print(f"[window-kernels] {kernel} {case}: max |kernel - model| / (u S) = {float(r.max()):.2f} "
          f"({float(frac.max()):.3f} of N u S)")
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and frac.max() <= 1.0, (kernel, case, float(frac.max()))


# ---- per-date kernels ------------------------------------------------------------------------

@pytest.mark.parametrize("offset", wm.OFFSETS)
@pytest.mark.parametrize("n", wm.NS)
@pytest.mark.parametrize("tmax", wm.TMAXES)
def test_per_date_kernels_on_complete_windows(device, tmax, n, offset):
    """pq_window_mean, pq_window_geomean, pq_window_sumsq (with and without mu), pq_cov_batched
    (mode 0 without the single row, mode 1) and pq_gram_xy_batched on the six-date table."""
    lib = _lib.load()
    R, y = wm.base_panel(n, offset)
    pan = _Panel(R, device, float("nan"), y)
    rows, tlen = wm.row_table(tmax)
    r_d, t_d = _dev(rows, device), _dev(tlen, device)
    B, ld = 6, _ld_of(n)
    W = [R[rows[d, :tlen[d]]] for d in range(B)]
    scale = np.abs(R).max()

    mu = _full((B, ld), FILL, device)
    _ok(lib.pq_window_mean(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, mu.data_ptr(), ld, None), lib)
    ge = _full((B, ld), FILL, device)
    _ok(lib.pq_window_geomean(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, ge.data_ptr(), ld, None), lib)
    mu_in = _full((B, ld), float("nan"), device)     # the centring input: the model's mean, rounded
    mu_in[:, :n] = _dev(np.stack([wm.mean(X).astype(np.float64) for X in W]), device)
    ssc, ss0 = _full((B, ld), FILL, device), _full((B, ld), FILL, device)
    _ok(lib.pq_window_sumsq(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, mu_in.data_ptr(), ld,
                            ssc.data_ptr(), ld, None), lib)
    _ok(lib.pq_window_sumsq(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, None, 0,
                            ss0.data_ptr(), ld, None), lib)
    two = np.flatnonzero(tlen >= 2)                   # mode 0 of a single row is 0 / 0: left out
    r2, t2, mu2 = _dev(rows[two], device), _dev(tlen[two], device), mu_in[_dev(two, device)].contiguous()
    S0 = _full((len(two), ld, ld), float("nan"), device)
    _ok(lib.pq_cov_batched(pan.ptr, pan.ldp, n, r2.data_ptr(), t2.data_ptr(), tmax, len(two), 0, mu2.data_ptr(), ld,
                           S0.data_ptr(), ld, ld * ld, None), lib)
    S1 = _full((B, ld, ld), float("nan"), device)
    _ok(lib.pq_cov_batched(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, 1, None, 0,
                           S1.data_ptr(), ld, ld * ld, None), lib)
    xty, yty = _full((B, ld), FILL, device), _full((B,), FILL, device)
    _ok(lib.pq_gram_xy_batched(pan.ptr, pan.ldp, n, pan.y.data_ptr(), r_d.data_ptr(), t_d.data_ptr(), tmax, B,
                               xty.data_ptr(), ld, yty.data_ptr(), None), lib)
    mu, ge, ssc, ss0, S0, S1, xty, yty = (v.cpu().numpy() for v in (mu, ge, ssc, ss0, S0, S1, xty, yty))

    for v in (mu, ge, ssc, ss0, xty):                  # columns past n are not the kernels' to write
        assert np.all(v[:, n:] == FILL)
    for d in range(B):
        X, yw = W[d], y[rows[d, :tlen[d]]]
        assert np.abs(wm.LD(1) * mu[d, :n] - wm.mean(X)).max() <= 1e-14 * scale, ("mean", d)
        assert wm.fro_rel(ge[d, :n], wm.geomean(X)) <= 1e-11, ("geomean", d)
        mc, m0 = wm.sumsq(X), wm.sumsq(X, False)
        assert np.all(np.abs(ssc[d, :n] - mc) <= 1e-12 * mc), ("sumsq centred", d)
        assert np.all(np.abs(ss0[d, :n] - m0) <= 1e-12 * m0), ("sumsq", d)
        if tlen[d] >= 2:
            k = int(np.searchsorted(two, d))
            assert wm.fro_rel(S0[k, :n, :n], wm.cov(X)) <= 1e-12, ("cov", d, wm.fro_rel(S0[k, :n, :n], wm.cov(X)))
            assert np.all(S0[k, n:, :] == 0) and np.all(S0[k, :, n:] == 0)
        assert wm.fro_rel(S1[d, :n, :n], wm.gram(X)) <= 1e-12, ("gram", d)
        assert np.all(S1[d, n:, :] == 0) and np.all(S1[d, :, n:] == 0)
        assert wm.fro_rel(xty[d, :n], wm.xty(X, yw)) <= 1e-12, ("X'y", d)
        assert abs(yty[d] - wm.yty(yw)) <= 1e-12 * wm.yty(yw), ("y'y", d)


@pytest.mark.parametrize("offset", wm.OFFSETS)
@pytest.mark.parametrize("n", wm.NS)
@pytest.mark.parametrize("tmax", wm.TMAXES)
def test_nan_aware_kernels(device, tmax, n, offset):
    """pq_window_nanmean (arithmetic, geometric) and pq_cov_pairwise_batched on windows with
    leading and trailing NaN runs, holes, an all-missing column and a pair of columns sharing
    one row: the NaN pattern of the reference, its values, zero padding."""
    lib = _lib.load()
    R = wm.nan_panel(n, offset)
    pan = _Panel(R, device, 1e300)
    rows, tlen = wm.row_table(tmax)
    r_d, t_d = _dev(rows, device), _dev(tlen, device)
    B, ld = 6, _ld_of(n)
    W = [R[rows[d, :tlen[d]]] for d in range(B)]
    scale = np.nanmax(np.abs(R))
    ma, mg = _full((B, ld), FILL, device), _full((B, ld), FILL, device)
    _ok(lib.pq_window_nanmean(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, ma.data_ptr(), ld, 0, None), lib)
    _ok(lib.pq_window_nanmean(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, mg.data_ptr(), ld, 1, None), lib)
    shift = np.zeros((B, ld))
    shift[:, :n] = np.stack([np.nan_to_num(wm.nanmean(X).astype(np.float64), nan=0.0) for X in W])
    shift[:, n:] = 1e300
    two = np.flatnonzero(tlen >= 2)                   # a single row has no covariance: left out
    r2, t2, sh = _dev(rows[two], device), _dev(tlen[two], device), _dev(shift[two], device)
    C = _full((len(two), ld, ld), FILL, device)
    _ok(lib.pq_cov_pairwise_batched(pan.ptr, pan.ldp, n, r2.data_ptr(), t2.data_ptr(), tmax, len(two), sh.data_ptr(), ld,
                                    C.data_ptr(), ld, ld * ld, None), lib)
    ma, mg, C = ma.cpu().numpy(), mg.cpu().numpy(), C.cpu().numpy()
    assert np.all(ma[:, n:] == FILL) and np.all(mg[:, n:] == FILL)
    for d in range(B):
        X = W[d]
        for got, geometric in ((ma[d, :n], False), (mg[d, :n], True)):
            m = wm.nanmean(X, geometric)
            miss = np.isnan(m.astype(np.float64))
            assert np.array_equal(np.isnan(got), miss) and miss[2], ("nanmean pattern", d, geometric)
            if geometric:
                assert wm.fro_rel(got[~miss], m[~miss]) <= 1e-11, ("nan geomean", d)
            else:
                assert np.abs(wm.LD(1) * got[~miss] - m[~miss]).max(initial=0.0) <= 1e-14 * scale, ("nanmean", d)
        if tlen[d] >= 2:
            k = int(np.searchsorted(two, d))
            ref = rp.cov_pairwise(X)
            got = C[k, :n, :n]
            miss = np.isnan(ref)
            assert np.array_equal(np.isnan(got), miss), ("pairwise pattern", d)
            assert miss[2].all() and (d > 0 or tmax < 2 or miss[3, 4])
            assert wm.fro_rel(got[~miss], ref[~miss]) <= 1e-12, ("pairwise", d, wm.fro_rel(got[~miss], ref[~miss]))
            assert np.all(C[k, n:, :] == 0) and np.all(C[k, :, n:] == 0)


# ---- sliding kernels -------------------------------------------------------------------------

@pytest.mark.parametrize("offset", wm.OFFSETS)
@pytest.mark.parametrize("n", wm.NS)
@pytest.mark.parametrize("cal,T", wm.SLIDE_CASES)
def test_slide_cov_on_planner_plans(device, cal, T, n, offset):
    """pq_cov_slide_batched, both modes, mirrored and lower_only, on slide_plan's own groups and
    shifts: every date within N u S of the longdouble value of what the kernel is given to
    compute, bitwise symmetric, zero padding, upper tiles untouched under lower_only."""
    lib = _lib.load()
    p = wm.plan(cal, T)
    wm.check_features(p)
    R = wm.base_panel(n, offset)[0]
    pan = _Panel(R, device, float("nan"))
    B, tmax, ld = p.B, p.rows.shape[1], _ld_of(n)
    r_d, t_d = _dev(p.rows, device), _dev(p.tlen, device)
    gs, sh = _dev(p.gstart, device), _dev(p.shift, device)
    tile = np.arange(ld) // 64
    upper = tile[:, None] < tile[None, :]
    for mode in (0, 1):
        m, model, N, S = wm.slide_model(cal, T, n, offset, mode)
        mu = _full((B, ld), float("nan"), device)
        mu[:, :n] = _dev(m, device)
        outs = []
        for lower_only in (0, 1):
            out = _full((B, ld, ld), float("nan"), device)
            _ok(lib.pq_cov_slide_batched(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, mode,
                                         mu.data_ptr() if mode == 0 else None, ld if mode == 0 else 0, out.data_ptr(),
                                         ld, ld * ld, gs.data_ptr(), len(p.gstart) - 1, sh.data_ptr(), lower_only,
                                         None), lib)
            outs.append(out.cpu().numpy())
        full, lo = outs
        _note(f"pq_cov_slide_batched mode {mode}", f"{cal} T={T} n={n} +{offset:g}", full[:, :n, :n], model, N, S)
        for d in range(B):
            assert np.array_equal(full[d, :n, :n], full[d, :n, :n].T), ("symmetry", mode, d)
            assert np.all(full[d, n:, :] == 0) and np.all(full[d, :, n:] == 0), ("padding", mode, d)
        assert np.array_equal(lo[:, ~upper], full[:, ~upper]) and np.isnan(lo[:, upper]).all()


@pytest.mark.parametrize("offset", wm.OFFSETS)
@pytest.mark.parametrize("n", wm.NS)
@pytest.mark.parametrize("cal,T", wm.GROUP_CASES)
def test_grouped_passes_on_planner_plans(device, cal, T, n, offset):
    """pq_window_moments_grouped, pq_window_geomean_grouped and pq_gram_xy_grouped (with and
    without dg) on GroupPlan(gmin=16)'s own groups, unions and offsets."""
    lib = _lib.load()
    p = wm.plan(cal, T)
    wm.check_features(p)
    R, y = wm.base_panel(n, offset)
    pan = _Panel(R, device, float("nan"), y)
    B, ld, G, umax = p.B, _ld_of(n), p.gp.ngroups, p.gp.umax
    t_d, gd, ur, uo = (_dev(a, device) for a in (p.tlen, p.gdates, p.urows, p.uoff))
    grp = (gd.data_ptr(), G, ur.data_ptr(), umax, uo.data_ptr(), t_d.data_ptr())
    tag = f"{cal} T={T} n={n} +{offset:g}"
    W = [R[p.window(b)] for b in range(B)]
    Wy = [y[p.window(b)] for b in range(B)]

    mu, dg = _full((B, ld), FILL, device), _full((B, ld), FILL, device)
    _ok(lib.pq_window_moments_grouped(pan.ptr, pan.ldp, n, *grp, mu.data_ptr(), ld, dg.data_ptr(), ld, None), lib)
    ge = _full((B, ld), FILL, device)
    _ok(lib.pq_window_geomean_grouped(pan.ptr, pan.ldp, n, *grp, ge.data_ptr(), ld, None), lib)
    xa, ya, da = _full((B, ld), FILL, device), _full((B,), FILL, device), _full((B, ld), FILL, device)
    _ok(lib.pq_gram_xy_grouped(pan.ptr, pan.ldp, n, pan.y.data_ptr(), *grp, xa.data_ptr(), ld, ya.data_ptr(),
                               da.data_ptr(), ld, None), lib)
    xb, yb = _full((B, ld), FILL, device), _full((B,), FILL, device)
    _ok(lib.pq_gram_xy_grouped(pan.ptr, pan.ldp, n, pan.y.data_ptr(), *grp, xb.data_ptr(), ld, yb.data_ptr(),
                               None, 0, None), lib)
    mu, dg, ge, xa, ya, da, xb, yb = (v.cpu().numpy() for v in (mu, dg, ge, xa, ya, da, xb, yb))
    for v in (mu, dg, ge, xa, da, xb):
        assert np.all(v[:, n:] == FILL)
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)      # dg is a by-product, not another path

    mu_m = np.stack([wm.mean(X) for X in W])
    N, Sm, Sd = wm.moments_bars(R, p, mu_m)
    _note("pq_window_moments_grouped mu", tag, mu[:, :n], mu_m, N, Sm)
    _note("pq_window_moments_grouped dg", tag, dg[:, :n], np.stack([wm.sumsq(X) for X in W]), N, Sd)
    ge_m = np.stack([wm.geomean(X) for X in W])
    Ng, Sg = wm.geomean_bars(R, p, ge_m)
    _note("pq_window_geomean_grouped", tag, ge[:, :n], ge_m, Ng, Sg)
    N, Sx, Sq, Ny, Sy = wm.gram_xy_bars(R, y, p)
    _note("pq_gram_xy_grouped X'y", tag, xa[:, :n], np.stack([wm.xty(X, yw) for X, yw in zip(W, Wy)]), N, Sx)
    _note("pq_gram_xy_grouped dg", tag, da[:, :n], np.stack([wm.sumsq(X, False) for X in W]), N, Sq)
    _note("pq_gram_xy_grouped y'y", tag, ya, np.array([wm.yty(yw) for yw in Wy]), Ny, Sy)


@pytest.mark.parametrize("T", [5, 30])
def test_minus_100_percent(device, T):
    """A return of exactly -1 in one column and of -1.5 in another, each entering and leaving
    windows inside one slide group: pq_window_geomean_grouped, pq_window_geomean and
    pq_window_nanmean(geometric) give -1.0 and NaN in exactly the windows that hold the row, the
    model everywhere else, and leave every other column as it is without the two returns.

    Before k_window_geomean_grp counted such entries instead of adding their logarithms, the sum
    kept -inf - (-inf) = NaN (or the NaN logarithm) after the row had left, and every later
    date of the group came out NaN in that column."""
    lib = _lib.load()
    n = 65
    R, c1, r1, c2, r2 = wm.minus100_case(T, n)
    p = wm.plan("weekday", T)
    B, ld, tmax = p.B, _ld_of(n), p.rows.shape[1]
    has1 = np.array([r1 in p.window(b) for b in range(B)])
    has2 = np.array([r2 in p.window(b) for b in range(B)])
    for has in (has1, has2):        # the row enters after its group's first date and leaves before its last
        hit = np.flatnonzero(has)
        g = np.searchsorted(p.gdates, hit[0], side="right") - 1
        assert len(hit) and p.gdates[g] < hit[0] and hit[-1] < p.gdates[g + 1] - 1
    model = np.stack([wm.geomean(R[p.window(b)]) for b in range(B)])
    mf = model.astype(np.float64)
    assert np.array_equal(mf[:, c1] == -1.0, has1) and np.array_equal(np.isnan(mf[:, c2]), has2)
    plain = mf != -1.0
    plain &= ~np.isnan(mf)

    r_d, t_d, gd, ur, uo = (_dev(a, device) for a in (p.rows, p.tlen, p.gdates, p.urows, p.uoff))
    grp = (gd.data_ptr(), p.gp.ngroups, ur.data_ptr(), p.gp.umax, uo.data_ptr(), t_d.data_ptr())
    got = {}
    for name, panel, poison in (("planted", R, float("nan")), ("clean", wm.base_panel(n)[0], float("nan")),
                                ("planted nan-aware", R, 1e300)):
        pan = _Panel(panel, device, poison)
        out = _full((B, ld), FILL, device)
        if poison != 1e300:
            _ok(lib.pq_window_geomean_grouped(pan.ptr, pan.ldp, n, *grp, out.data_ptr(), ld, None), lib)
            got["grouped " + name] = out.cpu().numpy()[:, :n]
            out = _full((B, ld), FILL, device)
            _ok(lib.pq_window_geomean(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, out.data_ptr(), ld,
                                      None), lib)
            got["per-date " + name] = out.cpu().numpy()[:, :n]
        else:
            _ok(lib.pq_window_nanmean(pan.ptr, pan.ldp, n, r_d.data_ptr(), t_d.data_ptr(), tmax, B, out.data_ptr(), ld, 1,
                                      None), lib)
            got["nanmean planted"] = out.cpu().numpy()[:, :n]
    others = np.ones(n, dtype=bool)
    others[[c1, c2]] = False
    N, S = wm.geomean_bars(R, p, model)
    for kernel in ("grouped", "per-date", "nanmean"):
        g = got[kernel + " planted"]
        print(f"[window-kernels] minus 100 % T={T} {kernel}: column {c1} = {g[:, c1].tolist()}")
        print(f"[window-kernels] minus 100 % T={T} {kernel}: column {c2} = {g[:, c2].tolist()}")
        assert np.array_equal(g[:, c1] == -1.0, has1), (kernel, "-1 exactly where the window holds the row")
        assert np.array_equal(np.isnan(g[:, c2]), has2), (kernel, "NaN exactly where the window holds the row")
        assert np.isnan(g).sum() == has2.sum(), (kernel, "no other NaN")
        if kernel == "grouped":
            _note("pq_window_geomean_grouped", f"minus 100 % T={T}", np.where(plain, g, 0.0), np.where(plain, model, 0.0), N, S)
            assert np.array_equal(g[:, others], got["grouped clean"][:, others])
        else:
            for b in range(B):
                assert wm.fro_rel(g[b, plain[b]], model[b, plain[b]]) <= 1e-11, (kernel, b)
            if kernel == "per-date":
                assert np.array_equal(g[:, others], got["per-date clean"][:, others])


def test_report_observed_units(device):
    """The largest |kernel - model| / (u S) of every sliding kernel over this module's cases
    (DESIGN.md records them next to N)."""
    for kernel in sorted(WORST):
        print(f"[window-kernels] {kernel:36s} max |kernel - model| / (u S) = {WORST[kernel][0]:8.2f}   "
              f"largest fraction of N u S = {WORST[kernel][1]:.3f}")
