"""The eigensolver's models (tests/jacobi_model.py) against closed forms, the float64
restatement of the kernel's algorithm on every named matrix (finite measures, convergence in
at most 20 of its 30 sweeps: a condition on the rotation rule, not a measurement), and the
device spacing helper of nearestPD against np.spacing.  No GPU."""
import functools

import numpy as np
import pytest
import torch

from porqua_amd.helper_functions import _spacing
from tests import jacobi_model as jm

LD = jm.LD
CASES = jm.cases()
IDS = [f"{name}-n{n}-ld{ld}" for name, n, ld, _ in CASES]


def test_ref_two_by_two_formula():
    a, b, d = 0.75, -1.25, 2.5
    lam, V = jm.jacobi_ref(np.array([[a, b], [b, d]]))
    h = np.hypot(LD(a - d) / 2, LD(b))
    ref = np.array([LD(a + d) / 2 - h, LD(a + d) / 2 + h])
    assert np.abs(np.sort(lam) - ref).max() <= 4 * np.finfo(LD).eps * abs(ref).max()
    assert np.abs(V.T @ V - np.eye(2)).max() <= 4 * np.finfo(LD).eps


@pytest.mark.parametrize("n", [5, 64, 97])
def test_ref_ring_adjacency(n):
    lam, V = jm.jacobi_ref(jm.matrix("ring", n))
    k = np.arange(n, dtype=LD)                                     # np.pi is pi to 1.2e-16 only
    ref = np.sort(2 * np.cos(2 * LD("3.14159265358979323846264338327950288") * k / n))
    assert np.abs(np.sort(lam) - ref).max() <= 1e-17
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-17


@pytest.mark.parametrize("n", [2, 65, 129])
def test_ref_ones(n):
    lam, V = jm.jacobi_ref(np.ones((n, n)))
    lam = np.sort(lam)
    assert abs(lam[-1] - n) <= 1e-17 * n and np.abs(lam[:-1]).max() <= 1e-17 * n
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-17


def test_ref_diagonal_is_returned_untouched():
    d = np.array([3.0, -1.0, 0.0, 1e-300, 2.5])
    lam, V = jm.jacobi_ref(np.diag(d))
    assert np.array_equal(lam, d.astype(LD)) and np.array_equal(V, np.eye(5, dtype=LD))


def test_ref_agrees_with_lapack_at_lapack_accuracy():
    A = jm.matrix("gauss", 97)
    lam, V = jm.jacobi_ref(A)
    ref = np.linalg.eigvalsh(A)
    assert np.abs(np.sort(lam) - ref).max() <= 97 * jm.U * np.abs(ref).max()
    r, o, e = jm.measures(A, lam, V, 97, lam)
    # ~10 sweeps of n - 1 rounds, one longdouble rounding each: 10 n u_ld = 1e-16, below u
    assert r <= 1e-16 and o <= 1e-16 and e == 0.0


@functools.lru_cache(maxsize=None)
def model(i):
    name, n, ld, A = CASES[i]
    ev, V, sweeps, conv = jm.block_jacobi_f64(A, n, ld, 30, 1e-14)
    return ev, V, sweeps, conv, jm.measures(A, ev, V, n)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_converges_within_20_sweeps(i):
    name, n, ld, A = CASES[i]
    ev, V, sweeps, conv, m = model(i)
    print(f"{IDS[i]}: sweeps {sweeps} resid {m[0] / jm.U:.0f}u orth {m[1] / jm.U:.0f}u eig {m[2] / jm.U:.0f}u")
    assert conv and sweeps <= 20, sweeps
    assert all(np.isfinite(m)), m
    # a correct eigendecomposition at all: far above any rounding, far below a wrong answer
    assert max(m) <= 1e-10, m
    assert np.all(ev[n:] == 0.0)
    assert np.array_equal(V[n:, n:], np.eye(ld - n)) and not V[:n, n:].any() and not V[n:, :n].any()
    if name in jm.NOTHING_TO_ROTATE or n == 1:
        assert sweeps == 1 and np.array_equal(ev[:n], np.diag(A)) and np.array_equal(V, np.eye(ld))


def test_spacing_matches_numpy_on_cpu_tensors():
    x = np.array([0.0, 5e-324, 1e-310, np.finfo(np.float64).tiny, 1e-300, 0.5, 1.0, 1.5, 2.0, 1e300])
    got = _spacing(torch.from_numpy(x)).numpy()
    assert np.array_equal(got, np.spacing(x)), (got, np.spacing(x))
    got0 = _spacing(torch.tensor(0.0, dtype=torch.float64))        # 0-d, as nearestPD uses it per matrix
    assert float(got0) == 5e-324
