"""The |q| floor of the initial rho inside k_init_state (pq_settings.rho0_qrel), through
pq_init_state and pq_init_state_lr called directly: rho must be torch.equal to the host formula
of engine._rho_floor_q,

    clamp(max(rho, rho0_qrel * max_i<n |q_i|), rho_min, rho_max),

applied to the rho the same entry point stores with rho0_qrel = 0.  Six problems, n = 70 at
ld = 128 (n is no multiple of a wave or of the block; [70, 128) is padding)."""
import ctypes

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from tests.test_gcap_gpu import _problem

pytestmark = pytest.mark.gpu

B, N, QREL = 6, 70, 10.0


def _q(device, ld):
    q = torch.zeros((B, ld), dtype=torch.float64, device=device)   # row 0: all zero
    q[1, N - 1] = 3.0                    # the only large entry is the last one below n
    q[2, :N] = 1e-3
    q[2, 7] = -4.5                       # a large negative entry
    q[3, :N] = 1e-3                      # floor 0.01 from the entries below n ...
    q[3, N] = 1e3                        # ... the padding (floor 1e4) is not read
    q[4, 3] = 1e9                        # floor above rho_max
    q[5, :N] = 1e-9                      # so small that rho_min wins (with rho_min above rho0)
    return q


def _dense(device):
    rng = np.random.default_rng(5)
    P = np.stack([np.diag(rng.uniform(0.5, 2.0, N) * (b + 1)) for b in range(B)])
    qb = engine.QPBatch.from_dense(P, np.zeros((B, N)), A=np.ones((1, N)), b=np.ones(1), lb=np.zeros(N),
                                   ub=np.ones(N), device=device)
    ws = engine.Workspace(qb)
    lib = _lib.load()

    def init(s, idx=None):
        args = (_ptr(idx), int(idx.numel())) if idx is not None else (None, 0)
        _lib.check(lib.pq_init_state(ctypes.byref(qb.c_struct()), ctypes.byref(ws.c_struct()), *args,
                                     ctypes.byref(s), engine._stream()), "pq_init_state")
    return qb, ws, init


def _window(device):
    qb, lr, _ = _problem(device, N, 20, B, 0.5)
    ws = engine.Workspace(qb, dense=False)
    lib = _lib.load()

    def init(s, idx=None):
        args = (_ptr(idx), int(idx.numel())) if idx is not None else (None, 0)
        _lib.check(lib.pq_init_state_lr(ctypes.byref(lr.c_struct()), ctypes.byref(qb.c_struct()),
                                        ctypes.byref(ws.c_struct()), *args, ctypes.byref(s), engine._stream()),
                   "pq_init_state_lr")
    return qb, ws, init


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _expected(base, q, st):
    qinf = q[:, :N].abs().amax(1)
    return torch.clamp(torch.maximum(base, st.rho0_qrel * qinf), st.rho_min, st.rho_max)


SETTINGS = {"rho0": dict(rho0_rel=0.0, rho0=0.1), "rho0_rel": dict(rho0_rel=4.0),
            "rho_min": dict(rho0_rel=0.0, rho0=0.1, rho_min=0.5)}


@pytest.fixture(scope="module", params=["dense", "window"])
def entry(request, device):
    qb, ws, init = (_dense if request.param == "dense" else _window)(device)
    assert qb.batch == B and qb.n == N and qb.ld == 128
    qb.q = _q(device, qb.ld)
    return qb, ws, init


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_floor_equals_the_host_formula(entry, name):
    qb, ws, init = entry
    st = engine.Settings(rho0_qrel=QREL, **SETTINGS[name])
    assert st.to_c().rho0_qrel == 0.0   # to_c() leaves the C field at 0: direct callers keep their rho
    init(st.to_c())
    base = ws.rho.clone()
    want = _expected(base, qb.q, st)
    init(st.to_c(rho0_qrel=QREL))
    torch.cuda.synchronize()
    print(name, "base", base.tolist(), "rho", ws.rho.tolist())
    assert torch.equal(ws.rho, want), (ws.rho.tolist(), want.tolist())
    # the cases are live: the floor moved rows 1, 2 and 4, row 4 sits at rho_max, row 3 ignored its padding
    assert bool((ws.rho[[1, 2, 4]] > base[[1, 2, 4]]).all()) and float(ws.rho[4]) == st.rho_max
    assert float(ws.rho[1]) == min(max(float(base[1]), 30.0), st.rho_max)
    assert float(ws.rho[3]) == max(float(base[3]), QREL * 1e-3, st.rho_min)   # (not QREL * 1e3: the padding)
    assert float(ws.rho[0]) == max(float(base[0]), st.rho_min)
    if name == "rho_min":
        assert float(base[5]) == 0.1 and float(ws.rho[5]) == 0.5
    # rho0_qrel = 0: rho is what it was without the field
    init(st.to_c(rho0_qrel=0.0))
    torch.cuda.synchronize()
    assert torch.equal(ws.rho, base)


def test_floor_on_an_index_list(entry, device):
    qb, ws, init = entry
    st = engine.Settings(rho0_qrel=QREL, rho0_rel=0.0, rho0=0.1)
    init(st.to_c())
    want = _expected(ws.rho.clone(), qb.q, st)
    ws.rho.fill_(-1.0)
    idx = torch.tensor([4, 1], dtype=torch.int32, device=device)
    init(st.to_c(rho0_qrel=QREL), idx)
    torch.cuda.synchronize()
    rho = ws.rho.cpu()
    assert rho[1] == want[1].cpu() and rho[4] == want[4].cpu(), rho.tolist()
    assert bool((rho[[0, 2, 3, 5]] == -1.0).all()), rho.tolist()


def test_nan_in_q_gives_nan_rho(entry):
    qb, ws, init = entry
    st = engine.Settings(rho0_qrel=QREL, rho0_rel=0.0, rho0=0.1)
    q0 = qb.q.clone()
    try:
        qb.q[2, 40] = float("nan")
        qb.q[5, N - 1] = float("nan")
        init(st.to_c())
        want = _expected(ws.rho.clone(), qb.q, st)   # torch.maximum and clamp propagate the NaN
        init(st.to_c(rho0_qrel=QREL))
        torch.cuda.synchronize()
        assert bool(torch.isnan(want[[2, 5]]).all()) and bool(torch.isnan(ws.rho[[2, 5]]).all()), ws.rho.tolist()
        assert torch.equal(ws.rho[[0, 1, 3, 4]], want[[0, 1, 3, 4]]), (ws.rho.tolist(), want.tolist())
    finally:
        qb.q.copy_(q0)
