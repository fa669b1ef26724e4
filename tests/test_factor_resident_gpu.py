"""The register-resident factor + inverse (chol_res.hip) behind pq_factor_batched: inverse against
numpy at the sizes where the 16 x 16 tiling changes shape, a capacitance-like ill-conditioned case,
non-PD reporting, the index list, and that the resident route is the one taken."""
import ctypes

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine

pytestmark = pytest.mark.gpu

ROUTE_RES = 2    # pq_factor_last_route(): 0 k_factor, 1 k_factor_sk, 2 k_factor_res
NMAX = 288       # PQ_RES_NMAX


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _spd(n, B, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((B, n + 7, n))
    return np.einsum("bki,bkj->bij", M, M) / n + 0.1 * np.eye(n)


def _factor(P, device, invert=2, idx=None, fill=None):
    """pq_factor_batched on the dense stack P (mg = 0, no box); returns (K (B, ld, ld), info, status, route)."""
    lib = _lib.load()
    B, n = P.shape[0], P.shape[1]
    qb = engine.QPBatch.from_dense(P, np.zeros((B, n)), device=device)
    s = engine.Settings(sigma=0.0).to_c()
    ws = engine.Workspace(qb)
    pb = qb.c_struct()
    pb.mg = 0
    pb.lb = pb.ub = None
    st = ws.c_struct()
    strm = engine._stream()
    _lib.check(lib.pq_init_state(ctypes.byref(pb), ctypes.byref(st), None, 0, ctypes.byref(s), strm), "init")
    if fill is not None:
        ws.K.fill_(fill)
    if idx is None:
        ip, ni = None, 0
    else:
        it = torch.tensor(idx, dtype=torch.int32, device=device)
        ip, ni = engine._ptr(it), len(idx)
    _lib.check(lib.pq_factor_batched(ctypes.byref(pb), ctypes.byref(st), ip, ni, ctypes.byref(s), invert, strm),
               "pq_factor_batched")
    lib.pq_factor_last_route.restype = ctypes.c_int
    route = int(lib.pq_factor_last_route())
    torch.cuda.synchronize()
    return ws.K.cpu().numpy(), ws.info.cpu().numpy(), ws.status.cpu().numpy(), route


@pytest.mark.parametrize("n", [16, 17, 31, 48, 65, 150, 284, NMAX])
def test_inverse_matches_numpy(device, n):
    P = _spd(n, 3, n)
    K, info, _, route = _factor(P, device, invert=2)
    assert route == ROUTE_RES
    assert not info.any()
    ld = K.shape[1]
    for b in range(3):
        err = _rel(K[b, :n, :n], np.linalg.inv(P[b]))
        print(f"n={n} b={b} rel err {err:.3e}")
        assert err <= 1e-10
        assert np.array_equal(K[b], K[b].T)
        # the padding holds the identity's inverse
        assert np.array_equal(K[b, n:, n:], np.eye(ld - n))
        assert not K[b, n:, :n].any() and not K[b, :n, n:].any()


def test_inverse_lower_only(device):
    """invert == 1: the lower triangle (what k_factor_sk defines) is the inverse's."""
    n = 150
    P = _spd(n, 3, 7)
    K, info, _, route = _factor(P, device, invert=1)
    assert route == ROUTE_RES and not info.any()
    for b in range(3):
        ref = np.linalg.inv(P[b])
        assert _rel(np.tril(K[b, :n, :n]), np.tril(ref)) <= 1e-10
        assert np.array_equal(np.tril(K[b])[n:, :], np.eye(K.shape[1])[n:, :])


def test_capacitance_like_ill_conditioned(device):
    n = 284
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 1000))
    G = X @ X.T
    hole = [5, 100, 177, 283]   # identity rows inside the valid range: a group with a short union
    G[hole, :] = 0.0
    G[:, hole] = 0.0
    a = (1e6 - 1.0) / np.linalg.eigvalsh(G)[-1]
    M = np.eye(n) + a * G
    assert 0.5e6 < np.linalg.cond(M) < 2e6
    K, info, _, route = _factor(M[None], device, invert=2)
    assert route == ROUTE_RES and info[0] == 0
    res_ref = np.abs(M @ np.linalg.inv(M) - np.eye(n)).max()
    res_gpu = np.abs(M @ K[0, :n, :n] - np.eye(n)).max()
    print(f"residual kernel {res_gpu:.3e} numpy {res_ref:.3e}")
    assert res_gpu <= 8.0 * res_ref + 1e-15
    for h in hole:
        e = np.zeros(n)
        e[h] = 1.0
        assert np.array_equal(K[0, h, :n], e) and np.array_equal(K[0, :n, h], e)


def test_non_pd_first_block(device):
    n = 150
    P = _spd(n, 3, 11)
    ref = [np.linalg.inv(P[b]) for b in range(3)]
    P[1] = -P[1]
    K, info, status, route = _factor(P, device, invert=2)
    assert route == ROUTE_RES
    assert info.tolist() == [0, 1, 0]
    assert status[1] == _lib.PQ_NON_CONVEX
    for b in (0, 2):
        assert _rel(K[b, :n, :n], ref[b]) <= 1e-10


def test_non_pd_later_block(device):
    n = 150
    P = _spd(n, 3, 12)
    ref = [np.linalg.inv(P[b]) for b in range(3)]
    P[2, 50, 50] = -1.0   # block column 3 (columns 48..63): the leading 48 x 48 block stays PD
    K, info, status, route = _factor(P, device, invert=2)
    assert route == ROUTE_RES
    assert info.tolist() == [0, 0, 1 + 16 * 3]
    assert status[2] == _lib.PQ_NON_CONVEX
    for b in (0, 1):
        assert _rel(K[b, :n, :n], ref[b]) <= 1e-10


def test_index_list(device):
    n = 65
    P = _spd(n, 5, 13)
    K, info, _, route = _factor(P, device, invert=2, idx=[3, 1], fill=float("nan"))
    assert route == ROUTE_RES and not info.any()
    for b in (1, 3):
        assert _rel(K[b, :n, :n], np.linalg.inv(P[b])) <= 1e-10
        assert np.array_equal(K[b], K[b].T)
    for b in (0, 2, 4):
        assert np.isnan(K[b]).all()
