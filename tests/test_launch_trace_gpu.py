"""Launch-trace pin of engine.solve_lowrank: which library entry points run, in which order,
on every route the host code can take (group capacitance, grouped fused / unfused, per-problem,
the sweep kernel with Cholesky and eigen capacitances, grouped and per-date polish, the
sync-free solve eager and replayed from HIP graphs, an adaptive-rho refactor round).

The library is wrapped in a recording proxy (``_lib.load`` monkeypatched): every ``pq_*`` call
appends its name and calls through.  The expected sequences (consecutive repeats written
``name*count``) and the result's capacitance / admm_launches / refactors / polish_fallbacks
were recorded on the commit before solve_lowrank was restructured around LowRankRoute; the
host code must reproduce each of them exactly.  Small shapes only: tests/test_gcap_gpu.py's
problem at n = 300, T = 60, D = 40 and the sweep batch n282-T20-L40-mg1 of
tests/test_admm_iterates_gpu.py."""

import pytest
import torch

from porqua_amd import _lib, engine
from tests.test_admm_iterates_gpu import ADAPT, STOP_CASE, _run_sweep
from tests.test_gcap_gpu import _problem

pytestmark = pytest.mark.gpu


class _Recorder:
    """The loaded library with every pq_* call recorded by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pq_"):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call

    def take(self):
        """The calls since the last take, run-length encoded."""
        out = []
        for c in self.calls:
            if out and out[-1][0] == c:
                out[-1][1] += 1
            else:
                out.append([c, 1])
        self.calls = []
        return tuple(n if k == 1 else "%s*%d" % (n, k) for n, k in out)


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


def _result(res):
    return (res.capacitance, res.admm_launches, res.refactors, res.polish_fallbacks)


def _slide(device, rec, steps=1, stream=False, graphs=False, settings=None, centred=True, caps=0, **kw):
    qb, lr, gp = _problem(device, 300, 60, 40, 0.2, centred=centred, caps=caps)
    ws = engine.Workspace(qb, dense=False)
    sg = engine.StageGraphs() if graphs else None
    if kw.pop("no_groups", False):
        gp = None
    out = []
    s = torch.cuda.Stream(device) if stream else torch.cuda.current_stream(device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        for _ in range(steps):
            rec.take()
            res = engine.solve_lowrank(qb, lr, settings, ws=ws, groups=gp, graphs=sg, **kw)
            torch.cuda.synchronize()
            assert bool(res.found.all())
            out.append((rec.take(), _result(res)))
    return out


def _sweep(device, rec, factor, settings):
    rec.take()
    sw, res, _ = _run_sweep(device, STOP_CASE, "sweep-eig" if factor == "eig" else "sweep-chol", settings)
    return [(rec.take(), _result(res))]


SLIDE = {
    "defaults": dict(),
    "gcap-off": dict(gcap=False),
    "fuse-off": dict(fuse=False),
    "groups-none": dict(no_groups=True),
    "grouped-polish-off": dict(grouped_polish=False),
    "caps8": dict(caps=8),
    "uncentred": dict(centred=False),
    "sync-free-eager": dict(sync_free=True, sf_rounds=4, stream=True, steps=3),
    "sync-free-graphs": dict(sync_free=True, sf_rounds=4, stream=True, steps=4, graphs=True),
    # a low fixed initial rho and a tight stop, adapted every 4 iterations: refactor rounds
    "adapt": dict(settings=engine.Settings(adapt_interval=4, eps_abs=1e-6, eps_rel=1e-6, rho0_rel=0.0, rho0=1e-5,
                                           rho0_qrel=0.0)),
}
SWEEP = {
    "sweep-chol": ("chol", {}),
    "sweep-eig": ("eig", {}),
    "sweep-chol-adapt": ("chol", ADAPT),
    "sweep-eig-adapt": ("eig", ADAPT),
}


def record(device, rec, name):
    """[(trace, (capacitance, admm_launches, refactors, polish_fallbacks)), ...] per step."""
    if name in SLIDE:
        return _slide(device, rec, **SLIDE[name])
    return _sweep(device, rec, *SWEEP[name])


_GCAP = ("pq_init_state_lr pq_lr_band_gram pq_gcap_assemble pq_factor_batched pq_gcap_prepare pq_admm_lr_gcap "
         "pq_polish_grouped_init ")
_REFACTOR = "pq_gcap_assemble pq_factor_batched pq_gcap_prepare pq_admm_lr_gcap "
# defaults: 8 rounds, then 3 dates handed back resume the ADMM and take the per-date polish
_DEFAULTS = (_GCAP + "pq_polish_grouped_round*8 pq_admm_lr_gcap pq_polish_w_batched", ("group", 2, 0, 3))
_PER_DATE = "pq_init_state_lr pq_lr_band_gram pq_lr_capacitance_band pq_factor_batched "
_GROUPED = _PER_DATE + "pq_admm_lr_grouped pq_polish_grouped_init pq_polish_grouped_round*4"
_SWEEP_CHOL = ("pq_window_mean pq_window_geomean pq_window_sumsq pq_init_state_lr pq_lr_band_gram "
               "pq_lr_capacitance_band pq_factor_batched pq_sweep_scratch_doubles pq_admm_lr_sweep ")
_SWEEP_EIG = ("pq_window_mean pq_window_geomean pq_window_sumsq pq_lr_capacitance pq_init_state_lr pq_lr_band_gram "
              "pq_eigcap_form pq_sweep_scratch_doubles pq_admm_lr_sweep ")

# per variant and step: (trace, (capacitance, admm_launches, refactors, polish_fallbacks))
EXPECTED = {
    "defaults": [_DEFAULTS],
    "gcap-off": [(_GROUPED, ("band", 1, 0, 0))],
    "fuse-off": [(_GROUPED, ("band", 1, 0, 0))],
    "groups-none": [(_PER_DATE + "pq_admm_lr_batched pq_polish_w_batched", ("band", 1, 0, 0))],
    "grouped-polish-off": [("pq_init_state_lr pq_lr_band_gram pq_gcap_assemble pq_factor_batched pq_gcap_prepare "
                            "pq_admm_lr_gcap pq_polish_w_batched", ("group", 1, 0, 0))],
    # the hand-backs' resumed ADMM asks for a new rho: one group refactor round inside the polish
    "caps8": [(_GCAP + "pq_polish_grouped_round*8 pq_admm_lr_gcap pq_polish_w_batched*2 pq_admm_lr_gcap " + _REFACTOR +
               "pq_polish_w_batched", ("group", 4, 15, 31))],
    # the wide rounds' own group capacitance, built once after k_pg_init
    "uncentred": [(_GCAP + "pq_gcap_assemble pq_factor_batched pq_gcap_prepare pq_polish_grouped_round*2",
                   ("group", 1, 0, 0))],
    # 4 rounds without a host check, then the flag path: the remaining rounds and the hand-backs
    "sync-free-eager": [_DEFAULTS] * 3,
    # (the first step fills the caches, the second captures, the later ones replay: only what runs
    # outside the captured stages is called, every time from the state the capture returned)
    "sync-free-graphs": [_DEFAULTS, _DEFAULTS] + 2 * [
        ("pq_init_state_lr pq_polish_grouped_round*4 pq_admm_lr_gcap pq_polish_w_batched", ("group", 2, 0, 3))],
    "adapt": [(_GCAP + "pq_polish_grouped_round*8 pq_admm_lr_gcap " + _REFACTOR * 4 + "pq_polish_w_batched",
               ("group", 6, 20, 5))],
    "sweep-chol": [(_SWEEP_CHOL + "pq_polish_grouped_init pq_polish_grouped_round*8 pq_sweep_scratch_doubles "
                    "pq_admm_lr_sweep pq_polish_w_batched*2 pq_sweep_scratch_doubles pq_admm_lr_sweep "
                    "pq_lr_capacitance_band pq_factor_batched pq_sweep_scratch_doubles pq_admm_lr_sweep "
                    "pq_polish_w_batched", ("band", 4, 2, 7))],
    "sweep-eig": [(_SWEEP_EIG + "pq_polish_grouped_init pq_polish_grouped_round*8 pq_polish_w_batched*2 "
                   "pq_sweep_scratch_doubles pq_admm_lr_sweep pq_eigcap_form pq_sweep_scratch_doubles "
                   "pq_admm_lr_sweep pq_polish_w_batched", ("eig", 3, 2, 3))],
    "sweep-chol-adapt": [(_SWEEP_CHOL + "pq_lr_capacitance_band pq_factor_batched pq_sweep_scratch_doubles "
                          "pq_admm_lr_sweep", ("band", 2, 80, 0))],
    "sweep-eig-adapt": [(_SWEEP_EIG + "pq_eigcap_form pq_sweep_scratch_doubles pq_admm_lr_sweep", ("eig", 2, 80, 0))],
}


@pytest.mark.parametrize("name", list(SLIDE) + list(SWEEP))
def test_launch_trace(device, rec, name):
    got = [(" ".join(trace), result) for trace, result in record(device, rec, name)]
    for step, g in enumerate(got):
        print("TRACE %s step %d: %s %s" % (name, step, g[1], g[0]))
    assert got == EXPECTED[name]
