"""k_gcap_assemble over its (group, 64 x 64 tile) grid: pq_gcap_assemble called directly on an M
prefilled with NaN, with the arguments of a real group-capacitance solve.

* Only the documented region is written: per group the lower 64-tiles with the diagonal tiles in
  full (row i: columns [0, 64 (i // 64 + 1))); everything else is still NaN.
* Beyond the U + mg capacitance rows the written part is the identity.
* Every written element is within 1 ulp of a numpy longdouble model built from the band Gram, pc
  and cc: M[i, j] = [i == j] + f t with the table entry t (band, pc or cc) and the factor f (c / d,
  sqrt(c) / d sqrt(R_r) or sqrt(R_r) sqrt(R_s) / d) formed in double in the kernel's order -- each
  of its steps is one correctly rounded operation -- and the last product and sum in longdouble.
  The kernel either contracts them into one FMA (the model's rounding) or rounds the product
  first, which moves the result by at most one more ulp.
* The one-workgroup-per-group form it replaces (PQ_GCAP_ASSEMBLE_OLD = 1, a process of its own:
  the switch is read once) writes the same M bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from tests.test_gcap_gpu import _problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (n, T, D, ub, stride, centred, budget, caps, cus)
CASES = {
    "centred-stride3": (300, 60, 30, 0.2, 3, True, True, 0, 256),        # the last group is shorter (2 of 4 dates)
    "uncentred-nobudget": (300, 60, 30, 0.2, 3, False, False, 0, 256),   # mg = 0
    "centred-caps8": (400, 120, 40, 0.05, 1, True, True, 8, 256),        # mg = 9: the wide (column-sparse) rows
    "uncentred-wide-groups": (400, 120, 40, 0.05, 1, False, True, 0, 2),   # few CUs: long groups, k_ld > 128
}


def assemble(device, name):
    """M (NaN-prefilled, then pq_gcap_assemble) of the case and what the model needs, as numpy arrays."""
    n, T, D, ub, stride, centred, budget, caps, cus = CASES[name]
    qb, lr, gp = _problem(device, n, T, D, ub, stride, centred=centred, budget=budget, caps=caps, cus=cus)
    st = engine.Settings(rho0_rel=0.0, rho0=0.01, rho0_qrel=0.0, adapt_interval=0, max_iter=3)
    ws = engine.Workspace(qb, dense=False)
    kept = {}
    band_setup = engine._band_setup

    def keep_band(*a, **kw):
        kept["bd"] = band_setup(*a, **kw)
        return kept["bd"]
    engine._band_setup = keep_band
    try:
        res = engine.solve_lowrank(qb, lr, st, ws=ws, groups=gp, polish=False)
    finally:
        engine._band_setup = band_setup
    torch.cuda.synchronize()
    assert res.capacitance == "group"
    gc, plan, bd = ws._gcap, ws.gcap_groups, kept["bd"]
    M = gc.buf["M"]
    M.fill_(float("nan"))
    s = st.to_c()
    _lib.check(_lib.load().pq_gcap_assemble(
        ctypes.byref(lr.c_struct()), ctypes.byref(qb.c_struct()), ctypes.byref(gc.c), ctypes.byref(s), *bd["cap"],
        bd["cc"].data_ptr(), engine._stream()), "pq_gcap_assemble")
    torch.cuda.synchronize()

    def host(t):
        return t.detach().cpu().numpy().copy()
    one = np.ones(qb.batch)
    return dict(M=host(M), mg=qb.mg, k_ld=int(gc.c.k_ld), gdates=host(plan.gdates), ucnt=host(plan.ucnt),
                urows=host(plan.urows).reshape(-1), umax=int(plan.umax), grho=host(gc.buf["grho"]),
                band=host(bd["band"]), r0=int(bd["r0"]), pc=host(bd["pc"]), cc=host(bd["cc"]),
                c=(host(qb.p_scale) if qb.p_scale is not None else one) *
                  (host(lr.w_scale) if lr.w_scale is not None else one),
                pd=host(qb.p_diag) if qb.p_diag is not None else 0.0 * one,
                lb0=float(qb.lb.reshape(-1)[0]), ub0=float(qb.ub.reshape(-1)[0]),
                lg=host(qb.lg).reshape(-1), ug=host(qb.ug).reshape(-1),
                sigma=st.sigma, rho_min=st.rho_min, eq_scale=st.eq_scale)


def _row_rho(lo, hi, rho, a):
    if lo == hi:
        return rho * a["eq_scale"]
    if np.isinf(lo) and np.isinf(hi):
        return a["rho_min"]
    return rho


def model(a, grp):
    """(written mask, longdouble model, U) of group grp's M_U."""
    k_ld, mg = a["k_ld"], a["mg"]
    U, d0, rho = int(a["ucnt"][grp]), int(a["gdates"][grp]), np.float64(a["grho"][grp])
    w = a["urows"][grp * a["umax"]: grp * a["umax"] + U].astype(np.int64) - a["r0"]
    c = np.float64(a["c"][d0])
    sqc = np.sqrt(np.maximum(c, 0.0))
    d = np.float64(a["sigma"]) + np.float64(a["pd"][d0]) + np.float64(_row_rho(a["lb0"], a["ub0"], rho, a))
    a1, a2 = c / d, sqc / d
    sr = np.array([np.sqrt(np.float64(_row_rho(a["lg"][r], a["ug"][r], rho, a))) for r in range(mg)])
    f = np.zeros((k_ld, k_ld))   # the factor (double, the kernel's order) and the table entry
    t = np.zeros((k_ld, k_ld))
    hi, lo = np.maximum(w[:, None], w[None, :]), np.minimum(w[:, None], w[None, :])
    f[:U, :U] = a1
    t[:U, :U] = a["band"][hi, hi - lo]
    if mg:
        pcw = a["pc"][w, :mg]                                    # (U, mg)
        f[U:U + mg, :U] = (a2 * sr)[:, None]
        t[U:U + mg, :U] = pcw.T
        f[:U, U:U + mg] = (a2 * sr)[None, :]
        t[:U, U:U + mg] = pcw
        f[U:U + mg, U:U + mg] = sr[:, None] * sr[None, :] / d
        t[U:U + mg, U:U + mg] = a["cc"].reshape(-1)[:mg * mg].reshape(mg, mg)
    want = np.eye(k_ld, dtype=np.longdouble) + f.astype(np.longdouble) * t.astype(np.longdouble)
    i, j = np.arange(k_ld)[:, None], np.arange(k_ld)[None, :]
    written = j < (i // 64 + 1) * 64
    return written, want, U


@pytest.mark.parametrize("name", sorted(CASES))
def test_assemble_region_padding_and_values(device, name):
    a = assemble(device, name)
    M, k_ld, mg = a["M"], a["k_ld"], a["mg"]
    G = len(a["ucnt"])
    sizes = np.diff(a["gdates"])
    print(name, "groups", G, "sizes", sizes.tolist(), "ucnt", a["ucnt"].tolist(), "mg", mg, "k_ld", k_ld)
    assert M.shape == (G, k_ld, k_ld) and k_ld % 64 == 0
    assert np.any(a["ucnt"] % 16 != 0)                       # a union size that is no multiple of 16
    if name == "centred-stride3":
        assert sizes[-1] < sizes[0] and a["ucnt"][-1] < a["ucnt"][0]   # a last group shorter than the others
    if name == "centred-caps8":
        assert mg == 9
    if name == "uncentred-wide-groups":
        assert k_ld > 128                                    # more than the three tiles of k_ld = 128
    worst = 0.0
    for grp in range(G):
        written, want, U = model(a, grp)
        got = M[grp]
        assert np.all(np.isnan(got[~written])), (name, grp, "written outside the lower 64-tiles")
        assert not np.any(np.isnan(got[written])), (name, grp, "a hole in the lower 64-tiles")
        k = U + mg
        pad = written.copy()
        pad[:k, :k] = False
        assert np.array_equal(got[pad], np.eye(k_ld)[pad]), (name, grp, "padding is not the identity")
        w64 = want.astype(np.float64)
        err = np.abs(got.astype(np.longdouble) - want)[written] / np.spacing(np.abs(w64))[written]
        worst = max(worst, float(err.max()))
        assert err.max() <= 1.0, (name, grp, float(err.max()), np.argwhere(written)[int(err.argmax())])
    print(name, "largest error %.3f ulp" % worst)


_CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from tests.test_gcap_assemble_grid_gpu import assemble
np.save(sys.argv[3], assemble(torch.device("cuda", torch.cuda.current_device()), sys.argv[2])["M"])
"""


@pytest.mark.parametrize("name", ["centred-caps8", "uncentred-wide-groups"])
def test_old_form_writes_the_same_matrix(device, name, tmp_path):
    new = assemble(device, name)["M"]
    out = str(tmp_path / "old.npy")
    env = dict(os.environ, PQ_GCAP_ASSEMBLE_OLD="1")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, out], check=True, env=env, cwd=ROOT, timeout=120)
    old = np.load(out)
    assert np.array_equal(new, old, equal_nan=True)
    assert not np.all(np.isnan(old))
