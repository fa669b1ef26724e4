"""Pass 0 of the grouped polish round (k_pg_passA<0>, k_pg_passB<0>, k_pg_post<0>): the product
w_scale (Xc'Xc x_B) of the variables at a non-zero bound, which pg_form_date takes into the
reduced right-hand side, and the round's bucket lists, which k_pg_post<0> clears and k_pg_form
fills.  The (n = 400, T = 120, 40 dates, ub = 0.05) problem of tests/test_gcap_gpu.py keeps
variables at their upper bound, so x_B != 0 and pass 0 is live.

Through the grouped polish, eager (host-driven rounds) and replayed (the sync-free stages as
HIP graphs): every status SOLVED, the weights of 8 dates against oracle.qp_ipm optima at the
bars of tests/test_headline_parity_gpu.py (weights 1e-5 L-inf, objective 1e-6 relative,
violation 1e-7), the window KKT certificate on all dates (1e-7), and after every round of the
eager solve the bucket lists hold each forming date exactly once, in the bucket of its free set."""
import numpy as np
import pytest
import torch

from oracle.qp_ipm import solve_qp
from porqua_amd import _lib, engine
from porqua_amd.workloads import window_certificate
from tests.test_gcap_gpu import _problem

pytestmark = pytest.mark.gpu

N, T, D, UB = 400, 120, 40, 0.05
DATES = [0, 5, 11, 17, 22, 28, 34, 39]
# record fields (porqua_amd/csrc/pg_record.h)
R_NZB, R_STATE, R_ROUNDS, R_W, R_KB, R_LIST, R_CNT, NBUCKET = 2, 3, 4, 320, 349, 352, 360, 6
BUCKET_MAX = (48, 64, 80, 96, 128)


class _RoundWatch:
    """The loaded library; around every pq_polish_grouped_round the record is read (two host syncs)."""

    def __init__(self, lib, ws):
        self._lib, self.ws, self.rounds = lib, ws, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "pq_polish_grouped_round":
            return fn

        def call(*a):
            torch.cuda.synchronize()
            before = self.ws.pg_record().cpu().numpy().copy()
            rc = fn(*a)
            torch.cuda.synchronize()
            self.rounds.append((before, self.ws.pg_record().cpu().numpy().copy()))
            return rc
        return call


@pytest.fixture(scope="module")
def problem(device):
    return _problem(device, N, T, D, UB)


@pytest.fixture(scope="module")
def oracle(problem):
    """(x, objective) of the oracle on DATES: P = 2 Xc'Xc / (T - 1) of each date's window."""
    qb, lr, _ = problem
    R, rows, mu = lr.panel.R.cpu().numpy(), lr.rows.cpu().numpy(), lr.mu.cpu().numpy()
    out = {}
    for d in DATES:
        Xc = R[rows[d, :T]][:, :N] - mu[d, :N]
        P = 2.0 / (T - 1) * Xc.T @ Xc
        sol = solve_qp(P, np.zeros(N), A=np.ones((1, N)), b=np.ones(1), lb=np.zeros(N), ub=np.full(N, UB))
        out[d] = (P, sol.x, 0.5 * sol.x @ P @ sol.x)
    return out


@pytest.fixture(scope="module")
def eager(problem):
    """The host-driven solve, the record read around every round: (result, workspace, watch)."""
    qb, lr, gp = problem
    ws = engine.Workspace(qb, dense=False)
    watch = _RoundWatch(_lib.load(), ws)
    load = _lib.load
    _lib.load = lambda: watch
    try:
        res = engine.solve_lowrank(qb, lr, None, ws=ws, groups=gp)
    finally:
        _lib.load = load
    torch.cuda.synchronize()
    assert res.capacitance == "group"
    return res, ws, watch


@pytest.fixture(scope="module")
def replayed(device, problem):
    """The sync-free solve from HIP graphs: the first step fills the caches, the second captures the
    stages, the later ones replay them."""
    qb, lr, gp = problem
    ws = engine.Workspace(qb, dense=False)
    sg = engine.StageGraphs()
    s = torch.cuda.Stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        for _ in range(4):
            res = engine.solve_lowrank(qb, lr, None, ws=ws, groups=gp, sync_free=True, graphs=sg)
            torch.cuda.synchronize()
    assert len(sg.graphs) >= 3, "no stage was captured"
    assert res.capacitance == "group"
    return res, ws, None


@pytest.fixture(scope="module", params=["eager", "replayed"])
def solved(request):
    return request.getfixturevalue(request.param)


def test_every_date_solved_and_certified(problem, solved):
    qb, lr, _ = problem
    res, _, _ = solved
    assert bool((res.status == _lib.PQ_SOLVED).all()), res.status.tolist()
    mg = qb.mg
    c = window_certificate(lr.panel.R, lr.rows, lr.tlen, lr.mu, qb.p_scale * lr.w_scale, qb.q[:, :N], res,
                           lb=qb.lb[0, :N], ub=qb.ub[0, :N], C=qb.Cg[0, :mg, :N], lg=qb.lg[0, :mg], ug=qb.ug[0, :mg])
    print(c)
    assert c["status_counts"] == {str(_lib.PQ_SOLVED): D}, c
    assert c["max_violation"] <= 1e-7, c
    assert c["max_rel_stationarity"] <= 1e-7, c
    assert c["max_rel_complementarity"] <= 1e-7, c


def test_weights_match_the_oracle_on_8_dates(solved, oracle):
    res = solved[0]
    x = res.x.cpu().numpy()
    at_ub = 0
    for d in DATES:
        P, xo, fo = oracle[d]
        xi = x[d]
        at_ub += int((xo > UB - 1e-9).sum())
        assert np.abs(xi - xo).max() <= 1e-5, (d, np.abs(xi - xo).max())
        obj = 0.5 * xi @ P @ xi
        assert abs(obj - fo) <= 1e-6 * abs(fo), (d, obj, fo)
        viol = max(abs(xi.sum() - 1.0), max(0.0, -xi.min()), max(0.0, xi.max() - UB))
        assert viol <= 1e-7, (d, viol)
    assert at_ub > 0   # variables at the upper bound: x_B != 0


def test_bucket_lists_hold_each_forming_date_once(eager):
    _, ws, watch = eager
    assert watch.rounds, "no grouped polish round ran"
    kbig = min(int(ws.ldk), 256)
    kmax = min(int(ws.ldk), 128)
    live = 0
    for r, (before, after) in enumerate(watch.rounds):
        pending = before[:, R_STATE] == _lib.PQ_PG_PENDING
        kb = after[:, R_KB].astype(np.int64)
        formed = (pending & (after[:, R_ROUNDS] == before[:, R_ROUNDS] + 1) & (after[:, R_W] == 0)
                  & (kb >= 1) & (kb <= kbig))
        live += int((formed & (after[:, R_NZB] != 0)).sum())
        cnt = after[0, R_CNT:R_CNT + NBUCKET].copy().view(np.int64)
        listed = []
        for bk in range(NBUCKET):
            dates = after[:cnt[bk], R_LIST + bk].astype(np.int64)
            for b in dates:
                want = next(i for i, m in enumerate(BUCKET_MAX) if kb[b] <= m) if kb[b] <= kmax else NBUCKET - 1
                assert want == bk, (r, int(b), int(kb[b]), bk)
            listed += dates.tolist()
        print("round", r, "pending", int(pending.sum()), "counts", cnt.tolist())
        assert len(listed) == len(set(listed)), (r, "a date is listed twice")
        assert sorted(listed) == np.nonzero(formed)[0].tolist(), (r, sorted(listed), np.nonzero(formed)[0].tolist())
    assert live > 0, "no forming date had x_B != 0: pass 0 was never live"
