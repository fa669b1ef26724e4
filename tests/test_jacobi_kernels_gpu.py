"""jacobi.hip against its models (tests/jacobi_model.py), through the C ABI with strides of the
test's choosing: pq_sym_eig_batched / pq_sym_eig_converged on the spectra PD repair exists for
(rank-deficient, clustered and repeated eigenvalues, exact zero rows, wide grading, zero
diagonals) and on every pairing / padding edge up to three block pairs, pq_psd_form_batched
and pq_tile_gemm_batched against longdouble products with derived bars, nearestPD_device on a
mixed batch against the reference's algorithm.

Bars.  The eigensolver's residual, orthogonality and eigenvalue error must each stay within
10 x the float64 restatement's value + 16 u (u = 2^-53): 10 is the project's margin between
two summation orders of the same algorithm (tests/test_admm_iterates_gpu.py), 16 u covers
one 2 x 2 rotation applied on both sides where the restatement happens to be exact.  The
product bars are derived in the model's docstring.  Run with ``-s`` for the kernel-to-model
ratios."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_pipeline as rp
from porqua_amd import _lib, engine
from porqua_amd import helper_functions as hf
from tests import jacobi_model as jm

pytestmark = pytest.mark.gpu

U = jm.U
SENT = 1.2345e77                                     # what the stride gaps hold before a call
CASES = jm.cases()
GROUPS = sorted({(n, ld) for _, n, ld, _ in CASES})


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def model(i):
    """The restatement's answer and both models' measures for case i, computed once."""
    name, n, ld, A = CASES[i]
    lam_ref = jm.jacobi_ref(A)[0]
    ev, V, sweeps, conv = jm.block_jacobi_f64(A, n, ld, 30, 1e-14)
    return dict(ev=ev, V=V, sweeps=sweeps, conv=conv, lam_ref=lam_ref, meas=jm.measures(A, ev, V, n, lam_ref))


def run_eig(mats, n, ld, max_sweeps=30, vectors=True, tol=1e-14):
    """pq_sym_eig_batched + pq_sym_eig_converged on the batch ``mats`` (n x n each) with NaN
    beyond n, strides beyond the matrices and poisoned gaps, which must come back untouched
    -> (evals (B, ld), V (B, ld, ld) or None, conv (B,))."""
    lib = _lib.load()
    B = len(mats)
    w = int(lib.pq_sym_eig_work_doubles(ld))
    sa = sv = ld * ld + 64
    se, sw = ld + 8, w + 16
    Ah = np.full((B, sa), SENT)
    for b, M in enumerate(mats):
        P = np.full((ld, ld), np.nan)
        P[:n, :n] = M
        Ah[b, :ld * ld] = P.ravel()
    A = torch.from_numpy(Ah).cuda()
    V = torch.full((B, sv), SENT, dtype=torch.float64, device="cuda") if vectors else None
    ev = torch.full((B, se), SENT, dtype=torch.float64, device="cuda")
    work = torch.full((B, sw), SENT, dtype=torch.float64, device="cuda")
    conv = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.pq_sym_eig_batched(A.data_ptr(), ld, sa, n, B, None if V is None else V.data_ptr(), sv,
                                      ev.data_ptr(), se, work.data_ptr(), sw, max_sweeps, tol, engine._stream()),
               "pq_sym_eig_batched")
    _lib.check(lib.pq_sym_eig_converged(work.data_ptr(), ld, sw, B, max_sweeps, conv.data_ptr(), engine._stream()),
               "pq_sym_eig_converged")
    torch.cuda.synchronize()
    assert bool((A[:, ld * ld:] == SENT).all()) and bool((ev[:, ld:] == SENT).all())
    assert bool((work[:, w:] == SENT).all())
    if V is not None:
        assert bool((V[:, ld * ld:] == SENT).all())
        V = V[:, :ld * ld].reshape(B, ld, ld).cpu().numpy()
    return ev[:, :ld].cpu().numpy(), V, conv.cpu().numpy()


# ----------------------------------------------------------------------------
# pq_sym_eig_batched / pq_sym_eig_converged
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("n,ld", GROUPS, ids=[f"n{n}-ld{ld}" for n, ld in GROUPS])
def test_sym_eig_against_the_models(device, n, ld):
    """Every case of one (n, ld) in one launch: padding, accuracy against the restatement,
    convergence within 30 sweeps, bitwise pass-through where nothing is to rotate."""
    idx = [i for i, c in enumerate(CASES) if (c[1], c[2]) == (n, ld)]
    ev, V, conv = run_eig([CASES[i][3] for i in idx], n, ld)
    eye = np.eye(ld)
    for b, i in enumerate(idx):
        name, _, _, A = CASES[i]
        m = model(i)
        tag = f"{name}-n{n}-ld{ld}"
        assert m["conv"], tag                                           # the model itself converged
        assert np.all(ev[b, n:] == 0.0), tag
        assert np.array_equal(V[b, n:, n:], eye[n:, n:]) and not V[b, :n, n:].any() and not V[b, n:, :n].any(), tag
        got = jm.measures(A, ev[b], V[b], n, m["lam_ref"])
        ratios = [g / r if r > 0 else (0.0 if g == 0 else np.inf) for g, r in zip(got, m["meas"])]
        print(f"{tag}: model sweeps {m['sweeps']}; resid/orth/eig kernel "
              + " ".join(f"{g / U:.0f}u" for g in got) + " model " + " ".join(f"{r / U:.0f}u" for r in m["meas"])
              + " ratio " + " ".join(f"{r:.2f}" for r in ratios))
        assert conv[b] == 1, tag
        for what, g, r in zip(("resid", "orth", "eig"), got, m["meas"]):
            assert np.isfinite(g) and g <= 10.0 * r + 16.0 * U, (tag, what, g / U, r / U)
        if m["sweeps"] == 1:                                            # nothing rotated
            assert np.array_equal(_bits(ev[b, :n]), _bits(np.diag(A).copy())), tag
            assert np.array_equal(_bits(V[b]), _bits(eye)), tag


def test_convergence_flag_on_both_parities(device):
    """gauss at n = 129 needs more than 3 sweeps and fewer than 29: the flag of the last
    queued sweep is read from either half of the flag buffer."""
    A = jm.matrix("gauss", 129)
    for sweeps, want in ((2, 0), (3, 0), (29, 1), (30, 1)):
        _, _, conv = run_eig([A], 129, 192, max_sweeps=sweeps)
        assert conv[0] == want, (sweeps, conv)


def test_convergence_flag_switches_with_the_last_sweep(device):
    """Far from the sweep that converges both halves of the flag buffer agree, so the flag is
    pinned at the transition itself: conv(m) = 1 exactly when sweep m - 1 rotated nothing,
    i.e. when m sweeps leave bitwise the eigenvectors of m - 1 sweeps.  Six spectra at n = 97
    that converge at different sweeps (6, 9, 4, 7, 2, 5 in the restatement) put the
    transition into either half of the buffer."""
    names = ("gauss", "cov", "ones", "rank2", "I+rank1", "ring")
    mats = [jm.matrix(s, 97) for s in names]
    runs = {m: run_eig(mats, 97, 128, max_sweeps=m) for m in range(1, 16)}
    first = []
    for b in range(len(mats)):
        for m in range(2, 16):
            same = np.array_equal(_bits(runs[m][1][b]), _bits(runs[m - 1][1][b]))
            assert runs[m][2][b] == int(same), (b, m, runs[m][2][b], same)
        first.append(min(m for m in range(1, 16) if runs[m][2][b] == 1))
    print("first max_sweeps that reports convergence at n = 97:", dict(zip(names, first)))
    assert {f % 2 for f in first} == {0, 1}, first


def test_mixed_batch_is_bitwise_the_matrices_alone(device):
    """Matrices that converge at different sweeps (at once, after a few, last) share a launch:
    each comes out bitwise as when solved alone; V = NULL gives bitwise the same eigenvalues."""
    n, ld = 66, 128
    mats = [jm.matrix(s, n) for s in ("diagonal", "ones", "gauss", "cov", "tiny_coupling")]
    ev, V, conv = run_eig(mats, n, ld)
    assert np.all(conv == 1)
    for b, M in enumerate(mats):
        e1, V1, c1 = run_eig([M], n, ld)
        assert np.array_equal(_bits(e1[0]), _bits(ev[b])) and np.array_equal(_bits(V1[0]), _bits(V[b])), b
        assert c1[0] == conv[b]
    e0, V0, c0 = run_eig(mats, n, ld, vectors=False)
    assert V0 is None and np.array_equal(_bits(e0), _bits(ev)) and np.array_equal(c0, conv)


# ----------------------------------------------------------------------------
# pq_psd_form_batched
# ----------------------------------------------------------------------------

LAMS = np.array([1.5, -2.0, 0.0, -0.0, 1e-200, -1e-200, 3e-3, 7.0])


@pytest.mark.parametrize("n", [33, 64, 65, 129])
def test_psd_form_elementwise_with_poisoned_padding(device, n):
    """out = V max(lam, 0) V' to (ld + 5) u S elementwise on the whole ld x ld output, with
    positive, negative, +0, -0 and tiny eigenvalues, V the solver's own and a random
    non-orthogonal one, NaN in V's columns k >= n and in evals[n:], strides beyond ld^2."""
    ld = jm.round_up(n, 64)
    lib = _lib.load()
    rng = np.random.default_rng(n)
    A = jm.matrix("gauss", n)
    ev, V, conv = run_eig([A], n, ld)
    assert conv[0] == 1
    crafted = LAMS[np.arange(ld) % len(LAMS)]
    Vs = np.stack([V[0], V[0], rng.normal(size=(ld, ld))])
    lam = np.stack([ev[0], crafted, crafted[::-1]])
    Vs[:, :, n:] = np.nan
    lam[:, n:] = np.nan
    sv, se, so = ld * ld + 64, ld + 8, ld * ld + 192
    Vh, eh = np.full((3, sv), SENT), np.full((3, se), SENT)
    Vh[:, :ld * ld] = Vs.reshape(3, -1)
    eh[:, :ld] = lam
    Vd, ed = torch.from_numpy(Vh).cuda(), torch.from_numpy(eh).cuda()
    out = torch.full((3, so), SENT, dtype=torch.float64, device="cuda")
    _lib.check(lib.pq_psd_form_batched(Vd.data_ptr(), sv, ed.data_ptr(), se, ld, n, 3, out.data_ptr(), so,
                                       engine._stream()), "pq_psd_form_batched")
    torch.cuda.synchronize()
    assert bool((out[:, ld * ld:] == SENT).all())
    got = out[:, :ld * ld].reshape(3, ld, ld).cpu().numpy()
    for b in range(3):
        ref, S = jm.psd_form_ref(Vs[b], lam[b], n)
        err = np.abs(got[b].astype(jm.LD) - ref)
        assert np.all(np.isfinite(got[b])), b
        worst = float((err / np.where(S > 0, S, 1)).max() / ((ld + 5) * U))
        print(f"psd_form n{n} b{b}: max err / ((ld + 5) u S) = {worst:.3f}")
        assert np.all(err <= (ld + 5) * U * S), (b, worst)


# ----------------------------------------------------------------------------
# pq_tile_gemm_batched
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("ld", [64, 128, 192])
def test_tile_gemm_all_transposes(device, ld):
    """C = op(A) op(B) to (ld + 1) u S elementwise for the four (ta, tb), on non-symmetric,
    distinct A and B, batch 3, three different strides beyond ld^2; C's gap untouched."""
    lib = _lib.load()
    rng = np.random.default_rng(ld)
    sa, sb, sc = ld * ld + 64, ld * ld + 128, ld * ld + 192
    Ah, Bh = np.full((3, sa), SENT), np.full((3, sb), SENT)
    Am, Bm = rng.normal(size=(3, ld, ld)), rng.normal(size=(3, ld, ld))
    Ah[:, :ld * ld], Bh[:, :ld * ld] = Am.reshape(3, -1), Bm.reshape(3, -1)
    Ad, Bd = torch.from_numpy(Ah).cuda(), torch.from_numpy(Bh).cuda()
    for ta in (0, 1):
        for tb in (0, 1):
            C = torch.full((3, sc), SENT, dtype=torch.float64, device="cuda")
            _lib.check(lib.pq_tile_gemm_batched(Ad.data_ptr(), sa, ta, Bd.data_ptr(), sb, tb, C.data_ptr(), sc, ld, 3,
                                                engine._stream()), "pq_tile_gemm_batched")
            torch.cuda.synchronize()
            assert bool((C[:, ld * ld:] == SENT).all())
            got = C[:, :ld * ld].reshape(3, ld, ld).cpu().numpy()
            for b in range(3):
                ref, S = jm.gemm_ref(Am[b], ta, Bm[b], tb)
                err = np.abs(got[b].astype(jm.LD) - ref)
                worst = float((err / S).max() / ((ld + 1) * U))
                print(f"tile_gemm ld{ld} ta{ta} tb{tb} b{b}: max err / ((ld + 1) u S) = {worst:.3f}")
                assert np.all(err <= (ld + 1) * U * S), (ta, tb, b, worst)


# ----------------------------------------------------------------------------
# nearestPD_device
# ----------------------------------------------------------------------------

def _pd_batch(n):
    """[(name, matrix, relative Frobenius bar against the reference's repair)]: the project's
    1e-12 where the input is PD or PSD-singular, 1e-10 where it is indefinite."""
    rng = np.random.default_rng(1000 + n)
    M = rng.normal(size=(n, n))
    K = rng.normal(size=(n, n))
    pd = M @ M.T / n + 0.1 * np.eye(n) + 1e-3 * (K - K.T)              # PD, not symmetric
    X = rng.normal(0, 0.02, size=(max(n // 3, 2), n))
    d = np.abs(rng.normal(size=n)) + 0.1
    d[n // 2] = -0.5
    # indefinite means eigenvalues of both signs (a small draw can be negative definite, whose
    # repair is rounding noise of the input and has no relative accuracy to speak of): draw
    # until the positive part is at least a tenth of the negative one.  n = 1 has no such matrix.
    G = M
    while True:
        ind = G + G.T - 2.0 * np.eye(n)
        w = np.linalg.eigvalsh(ind)
        if n == 1 or (w[0] < 0 and w[-1] >= 0.1 * -w[0]):
            break
        G = rng.normal(size=(n, n))
    return [("pd", pd, 1e-12), ("cov", np.cov(X, rowvar=False).reshape(n, n), 1e-12),
            ("indefinite", ind, 1e-10), ("neg_diag", np.diag(d), 1e-10),
            ("ones", np.ones((n, n)), 1e-12), ("zero", np.zeros((n, n)), 1e-12)]


@pytest.mark.parametrize("n", [1, 2, 64, 70])
def test_nearest_pd_mixed_batch(device, n, monkeypatch):
    batch = _pd_batch(n)
    unconverged = []
    orig = hf.sym_eig

    def counted(*a, **k):                              # every sym_eig call of the repair, not the last
        r = orig(*a, **k)
        unconverged.append(hf.sym_eig.last_unconverged)   # recorded on the module-level name
        return r

    monkeypatch.setattr(hf, "sym_eig", counted)
    A = torch.from_numpy(np.stack([m for _, m, _ in batch])).cuda()
    out_d = hf.nearestPD_device(A, n)
    assert hf.sym_eig.last_unconverged == 0 and unconverged and not any(unconverged), unconverged
    assert np.all(hf.pd_info_device(out_d, n).cpu().numpy() == 0)
    out = out_d[:, :n, :n].cpu().numpy()
    for b, (name, M, bar) in enumerate(batch):
        alone = hf.nearestPD_device(A[b:b + 1].clone(), n)[0, :n, :n].cpu().numpy()
        ref = rp.nearest_pd(M.copy())
        d_ref, n_ref = np.linalg.norm(out[b] - ref), np.linalg.norm(ref)
        d_alone, n_alone = np.linalg.norm(out[b] - alone), np.linalg.norm(alone)
        print(f"nearestPD n{n} {name}: |out - reference| {d_ref:.2e} of {n_ref:.2e} (bar {bar:.0e}), "
              f"|out - alone| {d_alone:.2e} of {n_alone:.2e}")
        assert d_ref <= bar * n_ref, (name, d_ref, n_ref)
        assert d_alone <= 1e-12 * n_alone, (name, d_alone, n_alone)
        if name == "pd":
            assert np.array_equal(_bits(out[b]), _bits((M + M.T) / 2))
        if name == "zero":
            dg = np.diag(out[b])
            print(f"nearestPD n{n} zero: diagonal {dg.min()!r} .. {dg.max()!r}")
            assert not (out[b] - np.diag(dg)).any() and np.all(dg > 0) and np.all(dg <= 2.0 ** -53)
    assert not any(unconverged), unconverged
