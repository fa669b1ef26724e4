"""The sync-free flag (ws._sf_flag) comes from the grouped polish itself: k_pg_post sets the record
field PQ_PG_SFLAG when its round leaves a date for the host-driven repairs.  Right after the
sync-free stage (solve_lowrank's host_work hook runs there, before the flag is read and before
any repair touches the record) the device flag must equal the five-condition torch expression
(engine.sf_flag_torch) on the same record and status: state PENDING or FALLBACK, status
NEED_REFACTOR, SOLVED_INACCURATE or UNSOLVED."""
import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from porqua_amd.workloads import MinVarianceBacktest
from tests.test_gcap_gpu import _problem

pytestmark = pytest.mark.gpu


def _flag_after_stage(device, qb, lr, gp, settings, rounds):
    """(device flag, torch expression, count field) right after the sync-free stage, on a side stream."""
    ws = engine.Workspace(qb, dense=False)
    snap = {}

    def host_work():
        torch.cuda.synchronize()
        rec = ws.pg_record()
        snap["flag"] = bool(ws._sf_flag.item())
        snap["want"] = bool(engine.sf_flag_torch(rec, ws.status).item())
        snap["count"] = int(rec[0, _lib.PQ_PG_SFLAG:_lib.PQ_PG_SFLAG + 1].view(torch.int64).item())
        st_pg, st = rec[:, _lib.PQ_PG_STATE], ws.status
        snap["left"] = int(((st_pg == _lib.PQ_PG_PENDING) | (st_pg == _lib.PQ_PG_FALLBACK) |
                            (st == _lib.PQ_NEED_REFACTOR) | (st == _lib.PQ_SOLVED_INACCURATE) |
                            (st == _lib.PQ_UNSOLVED)).sum().item())
        snap["status"] = np.bincount(st.cpu().numpy(), minlength=5).tolist()

    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        res = engine.solve_lowrank(qb, lr, settings, ws=ws, groups=gp, sync_free=True, sf_rounds=rounds,
                                   host_work=host_work)
        torch.cuda.synchronize()
    assert snap, "the sync-free route was not taken"
    print(rounds, snap)
    return snap, res


@pytest.fixture(scope="module")
def cases(device):
    """Every case once: the (300, 60, 40, ub 0.2) slide at 1, 4 and 8 rounds; the same with max_iter = 1 (the
    ADMM stops unconverged -- measured: every status is MAX_ITER, not UNSOLVED, when the polish stage ends, and
    the polish hands every date back); with an adaptive rho that asks for a refactorisation (statuses
    NEED_REFACTOR, which the sync-free solve leaves to the flag); and a batch the rounds finish completely
    (minimum variance, n = 1000, T = 252, 64 dates)."""
    slide = _problem(device, 300, 60, 40, 0.2)
    out = {r: _flag_after_stage(device, *slide, None, r) for r in (1, 4, 8)}
    out["max_iter=1"] = _flag_after_stage(device, *slide, engine.Settings(max_iter=1), 4)
    adapt = engine.Settings(adapt_interval=4, eps_abs=1e-6, eps_rel=1e-6, rho0_rel=0.0, rho0=1e-5, rho0_qrel=0.0,
                            eps_grouped=0.0)   # (no loose stop: the ADMM runs into its first rho adaptation)
    out["adapt"] = _flag_after_stage(device, *slide, adapt, 4)
    wl = MinVarianceBacktest(D=64, device=device)
    out["finished"] = _flag_after_stage(device, wl.qb, wl.lr, wl.gplan, wl.settings, 8)
    return out


@pytest.mark.parametrize("case", [1, 4, 8, "max_iter=1", "adapt", "finished"])
def test_flag_equals_the_torch_expression(cases, case):
    snap, res = cases[case]
    assert snap["flag"] == snap["want"], snap
    assert snap["count"] == (1 if snap["left"] else 0), snap   # (the field itself, read as int64)
    if case not in ("max_iter=1", "adapt"):
        assert bool((res.status == _lib.PQ_SOLVED).all())   # the repairs behind a set flag finished the rest


def test_unconverged_statuses_set_the_flag(cases):
    snap, _ = cases["max_iter=1"]
    assert snap["flag"] and snap["status"][_lib.PQ_SOLVED] == 0, snap   # (no date converged)
    snap, _ = cases["adapt"]
    assert snap["flag"] and snap["status"][_lib.PQ_NEED_REFACTOR] > 0, snap


def test_a_finished_polish_clears_the_flag(cases):
    snap, _ = cases["finished"]
    assert snap["left"] == 0 and snap["count"] == 0 and not snap["flag"], snap


def test_both_truth_values_occurred(cases):
    assert {snap["flag"] for snap, _ in cases.values()} == {True, False}
