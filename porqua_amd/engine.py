"""Device engine: batched covariance + batched dense QP solve on MI355X through the C ABI.

Host code only stages data (PyTorch-ROCm tensors for device memory and the current HIP
stream) and drives the kernels of ``libporqua_hip.so``:

  K1 pq_window_mean / pq_cov_batched / pq_gram_xy_batched / pq_window_geomean
  K2 pq_factor_batched   (KKT formation + Cholesky [+ inverse])
  K3 pq_admm_batched     (OSQP-style ADMM, per-problem convergence)
  K4 pq_polish_batched   (active-set polish + exact residuals)

There is deliberately no CPU fallback: without the library or a GPU every entry point
raises ``PorquaHipError``.
"""
from __future__ import annotations

import os
import ctypes
import dataclasses
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

F64 = torch.float64


def round_up(v: int, m: int) -> int:
    return ((int(v) + m - 1) // m) * m


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.PorquaHipError("no HIP device visible: the MI355X engine has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


@dataclass
class Settings:
    """ADMM / polish settings.  OSQP defaults except a scale-aware initial rho (4 x mean
    diag P, adapted every 60 iterations: no refactorisation on the n = 1000 min-variance
    windows, tests/engine_model.py), the stopping tolerance and the polish settings.  ADMM
    only has to reach an approximate point whose active set the polish can correct: measured
    on config 3 (round 2 kernels, bench.py --set eps_abs=... eps_rel=...) eps 2e-3 gives 20 ADMM iterations +
    2.7 polish rounds against 21 + 2.6 at 1e-3 and 18 + 2.9 at 4e-3 (about 2 % apart; configs
    2, 4 and 5 also gain), alpha 1.7 / 1.8 trade 10 / 29 more ADMM iterations for 0.7 / 1.5
    fewer polish rounds and lose; round 1 measured 1e-3 against 1e-4 (95.7k vs 85.1k QPs/s).
    Every answer is still KKT-checked and a rejected polish resumes ADMM to eps_retry.
    Passed through ``params`` of the reference API."""
    rho0: float = 0.1
    rho0_rel: float = 4.0      # initial rho = rho0_rel * mean(diag P) (0: use rho0)
    sigma: float = 1e-6
    alpha: float = 1.6
    eps_abs: float = 2e-3      # ADMM stop before the polish (twice OSQP's default; the polish
    eps_rel: float = 2e-3      # identifies the active set and solves the reduced KKT exactly)
    eps_retry: float = 1e-7    # problems whose polish is rejected resume ADMM to this eps
    rho_min: float = 1e-6
    rho_max: float = 1e6
    adapt_tol: float = 5.0
    eq_scale: float = 1e3
    delta: float = 1e-9        # polish regularisation, relative to the problem scale
    dual_tol: float = 1e-9     # multiplier sign tolerance, relative to the problem scale
    max_iter: int = 4000
    adapt_interval: int = 60
    polish: int = 1
    polish_rounds: int = 8
    refine_iters: int = 1      # proximal refinement steps per polish round (then KKT-checked)
    # problems whose polish is rejected are polished again with this many refinement steps
    # (nearly singular P_FF, e.g. small risk aversions) before the ADMM retry (host-side)
    refine_retry: int = 4
    # initial rho >= rho0_qrel * max|q|: for nearly linear objectives (small risk aversion) 4
    # mean(diag P) is far too small a rho.  to_c() leaves pq_settings.rho0_qrel at 0: only the
    # init call of solve / solve_lowrank passes it (k_init_state then applies the floor), so
    # every other caller of the init entry points keeps its rho
    rho0_qrel: float = 10.0
    # wide rounds of the grouped polish (polish_gw.hip, host-side): refinement steps per round
    # (early exit at the 1e-13 residual) and the group capacitance's diagonal relative to the
    # problem scale (the reduced KKT system keeps delta).  Measured on config 4
    # (profiles/r03c_config4_grid.log, steps 2/4/6/10 x 1e-9/1e-7): at 1e-9 the explicit M_U^-1
    # (condition ~1e11) limits each step to ~1e-5, so 2 steps leave 2e-7 stationarity and 1.8
    # rounds; 1e-7 converges in <= 4 steps to 5e-13 (87k QPs/s, polish 40 ms, 1.0 rounds)
    refine_wide: int = 6
    delta_wide: float = 1e-7
    # centred windows (mean-variance family) on the group capacitance with the grouped polish
    # (host-side): the ADMM stops at this looser eps -- it only has to predict the active
    # set, the pipeline's rounds are cheap and every answer is certified -- and the dates the
    # pipeline hands to the per-date polish resume ADMM to eps_abs / eps_rel first (their
    # rounds are not cheap).  Measured (profiles/r03s_*, r03t_*, r03u_*): config 3 2e-3 /
    # 1e-2 / 2e-2 / 1e-1 -> 311k / 335k / 343k / 353k QPs/s (20 / 16 / 15 / 11 iterations,
    # 2.7 / 3.1 / 3.2 / 3.8 rounds); with the sparse exact-P x pass (r03y_*) 2e-2 / 3e-2 /
    # 5e-2 / 1e-1 -> 347k / 357k / 358k / 360k at 5 / 5 / 6 / 6 rounds at most (of the 8
    # allowed): 3e-2 keeps the round count of 2e-2; with polish_fix_rel = 0.05 (r03Q_grid*):
    # 3e-2 / 5e-2 -> 374k / 389k at 2.86 / 2.99 rounds, at most 5 / 5.  Round 4, with the
    # inner primal steps (polish_inner) the rounds stay cheap from a looser point
    # (profiles/r04t_eg*.log, one box, polish_inner = 1): 0.2 / 0.3 -> 461k / 466k (9 / 8
    # iterations, 2.2 / 2.3 rounds, at most 4, largest free set 88); 0.5 and 1.0 stop after 4
    # iterations -- ADMM's residuals are not monotone: they dip below 0.5 at iteration 4 and
    # stay above 0.3 until 8 -- where the free sets outgrow the LDS solve and every date takes
    # the per-date fallback (144k).  The loose stop therefore also waits for min_iter_grouped
    # iterations: 0.3 with at least 8 -> 536k (r04O_eg25*.log: 0.25, the same 8 iterations),
    # and a larger eps cannot fall off that cliff.  Tracking (uncentred) windows keep eps_abs: their free
    # sets mostly exceed the LDS solve -- config 2 53.0k at 2e-3, 45.0k at 1e-2 from the loose
    # point, 50.1k with the resume; config 4 87.9k / 91.8k / 87.6k.  0 or <= eps_abs: off.
    # Round 6, with the register-tile polish solve (profiles/r06p_*, r06q_*): (0.3, floor 8) ->
    # 676-680k QPs/s (ADMM 2.90, polish 2.52-2.61 ms); (0.5 or 1.0, floor 7) -> 694-699k (7
    # iterations: ADMM 2.56, polish 2.75 ms, 2.27 rounds, at most 4); floor 6 or 5 -> 525-560k
    # (polish 5.0-5.3 ms: free sets beyond the register solve and up to 5 rounds).  So the loose
    # stop is in effect a 7-iteration warm start of the polish for the centred windows
    eps_grouped: float = 0.5
    # (host-side) the loose stop's pq_settings.min_iter.  Round 5 (profiles/r05T_config3_miniter_grid.log):
    # 6 / 7 / 8 / 9 -> the same 8 iterations below 9 (eps 0.3 is first met at 8), 9 slower (569k);
    # round 6: 7 with eps 0.5 (above)
    min_iter_grouped: int = 7
    # (host-side) the same loose stop for uncentred (tracking) windows on the group capacitance;
    # 0: off (they stop at eps_abs / eps_rel).  Measured on config 2 (profiles/r04T_*.log): off /
    # 1e-2 / 3e-2 / 1e-1 -> 161k / 151k / 142k / 114k QPs/s (20 / 17 / 15 / 13 iterations, 2.7 /
    # 3.1 / 3.5 / 4.0 rounds): the tracking rounds (free sets of 160..220) cost more than the
    # ADMM iterations they replace
    eps_grouped_tracking: float = 0.0
    # (host-side) small batches of tracking windows (at most small_batch dates, e.g. the
    # reference notebook's 13-date monthly run) take the loose stop at this eps when it is > 0
    # and eps_grouped_tracking is 0.  Off by default: the first grid on the 13-date monthly run
    # (profiles/r05N_monthly_grid.log: off / 3e-3 / 1e-2 / 3e-2 / 0.1 / 0.3 -> 10.3 / 10.4 / 9.5 /
    # 9.6 / 10.0 / 9.5 ms) did not hold up when re-measured as medians of five
    # (profiles/r05V_monthly_grid.log: 1e-2 9.84 ms, off 9.78 ms).  The rule keys on the batch
    # of one solve call, so in a chunked backtest only a short last chunk would take it
    eps_grouped_tracking_small: float = 0.0
    small_batch: int = 64
    # (host-side) tracking windows with more than 4 general rows (the column-sparse wide form,
    # e.g. config 4's sector caps) take the loose stop at this eps when eps_grouped_tracking is
    # 0: their polish finishes in about one wide round, so ADMM iterations are the cost.
    # Measured on config 4 (profiles/r05Q_grid.log): off / 3e-3 / 1e-2 / 3e-2 -> 119-123k /
    # 124k / 129k / 113k QPs/s (20 / 19 / 17 / 15 iterations; 3e-2 hands dates to the per-date
    # polish); around it (profiles/r05U_config4_eps_wide_grid.log) 1e-2 / 1.5e-2 / 2e-2 ->
    # 130-131k / 122-124k / 128-131k (1.00 / 1.12 / 1.05 rounds: 1e-2 the steadiest); config 2
    # (one general row) keeps eps_abs (round 4: 161k off, 151k at 1e-2;
    # round 5, profiles/r05S_config2_loose_grid.log: off / 3e-3 / 1e-2 -> 227k / 226-230k /
    # 214-217k: its rounds of free sets of ~190 still cost more than the iterations saved)
    eps_grouped_tracking_wide: float = 1e-2
    # (host-side) the loose stop also on the per-problem capacitance (grouped ADMM without the
    # group capacitance: the lambda sweep, whose problems of a date differ in P's scale)
    eps_grouped_percap: bool = False
    min_iter: int = 0           # pq_settings.min_iter: no convergence test before this iteration
    # grouped polish: variables with x - lb < polish_fix_rel * max(x - lb) at the ADMM point
    # also start fixed at lb (besides OSQP's z - lb < -y): the loose ADMM point leaves small
    # positive weights that the first rounds would only fix later.  Numpy model of config 3
    # (tests/engine_model.py, eps 3e-2, 10 dates): 0 / 0.05 / 0.1 / 0.2 -> 3.0 / 2.6 / 2.3 /
    # 3.3 rounds, first free sets 79 / 71 / 62 / 47 (wrong fixes cost the rounds back); on
    # the GPU (profiles/r03N_*): 0 / 0.05 / 0.1 -> 363k / 378k / 372k QPs/s, 3.31 / 2.86 / 3.0
    # rounds on average, at most 5 / 5 / 6.  Round 4 at eps_grouped 0.2 / 0.3 with one inner
    # step: 0.05 / 0.1 -> 461k / 467k and 466k / 479k (profiles/r04t_eg*_in1{,_fr1}.log).
    # Centred windows only (k_pg_init)
    polish_fix_rel: float = 0.1
    # grouped polish, LDS solve (k_pg_solve): free variables outside their box are fixed at
    # it and the reduced system re-solved inside the round, up to this many times per round,
    # instead of one whole round (window passes, checks, setup) per such step.  Measured at
    # eps_grouped 0.3 (profiles/r04t_eg3_in{1,2}.log): 1 / 2 -> 466k / 457k QPs/s (2.29 / 2.11
    # rounds; the second step costs more in the solve buckets than the rounds it saves)
    polish_inner: int = 1
    # grouped polish: a rejected round also releases the variables at a bound whose multiplier
    # is within this fraction of the problem scale of the wrong sign (0: off; see pq_settings)
    polish_release_rel: float = 0.0

    def to_c(self, **override) -> _lib.PQSettings:
        """The C settings struct, with ``override`` replacing fields (derived settings of one solve)."""
        return _lib.PQSettings(**{**{k: getattr(self, k) for k in _C_SETTINGS}, **override})

    @classmethod
    def from_params(cls, params) -> "Settings":
        s = cls()
        if params:
            for f in dataclasses.fields(cls):
                for key in (f.name, "admm_" + f.name):
                    if key in params and params[key] is not None:
                        v, typ = params[key], type(getattr(s, f.name))
                        if typ is bool and isinstance(v, str):   # "0" / "false" from --set KEY=VALUE
                            v = v.strip().lower() not in ("0", "false", "no", "off", "")
                        setattr(s, f.name, typ(v))
        return s


_C_SETTINGS = tuple(c[0] for c in _lib.PQSettings._fields_
                    if c[0] in Settings.__dataclass_fields__ and c[0] != "rho0_qrel")   # (not host-side)


# ----------------------------------------------------------------------------------------
# Problem batches
# ----------------------------------------------------------------------------------------


class QPBatch:
    """A batch of dense QPs  min 0.5 x'(ps P + pd I)x + q'x  s.t. lg <= Cg x <= ug,
    lb <= x <= ub, laid out as include/porqua_hip.h expects (ld = round_up(n, 64))."""

    def __init__(self, n: int, batch: int, mg: int, device=None, shared_constraints=True,
                 has_box=True, P=None):
        self.device = device or default_device()
        self.n, self.batch, self.mg = int(n), int(batch), int(mg)
        self.ld = round_up(max(n, 1), 64)
        self.mg_pad = round_up(max(mg, 1), 8)
        ld, dev = self.ld, self.device
        self.P = P if P is not None else torch.zeros((batch, ld, ld), dtype=F64, device=dev)
        self.q = torch.zeros((batch, ld), dtype=F64, device=dev)
        self.p_scale = None
        self.p_diag = None
        nc = 1 if shared_constraints else batch
        self.shared = shared_constraints
        self.Cg = torch.zeros((nc, max(mg, 1), ld), dtype=F64, device=dev)
        self.lg = torch.full((nc, max(mg, 1)), -np.inf, dtype=F64, device=dev)
        self.ug = torch.full((nc, max(mg, 1)), np.inf, dtype=F64, device=dev)
        self.has_box = has_box
        if has_box:
            self.lb = torch.full((nc, ld), -np.inf, dtype=F64, device=dev)
            self.ub = torch.full((nc, ld), np.inf, dtype=F64, device=dev)
        else:
            self.lb = self.ub = None

    def c_struct(self) -> _lib.PQProblem:
        ld = self.ld
        cs = 0 if self.shared else self.Cg.stride(0)
        gs = 0 if self.shared else self.lg.stride(0)
        bs = 0 if (self.shared or not self.has_box) else self.lb.stride(0)
        return _lib.PQProblem(
            n=self.n, ld=ld, batch=self.batch, mg=self.mg,
            P=None if self.P is None else self.P.data_ptr(),
            P_stride=0 if self.P is None else self.P.stride(0),
            p_scale=None if self.p_scale is None else self.p_scale.data_ptr(),
            p_diag=None if self.p_diag is None else self.p_diag.data_ptr(),
            q=self.q.data_ptr(), q_stride=self.q.stride(0),
            Cg=self.Cg.data_ptr(), Cg_stride=cs,
            lg=self.lg.data_ptr(), ug=self.ug.data_ptr(), g_stride=gs,
            lb=None if self.lb is None else self.lb.data_ptr(),
            ub=None if self.ub is None else self.ub.data_ptr(), box_stride=bs)

    @classmethod
    def from_dense(cls, P, q, A=None, b=None, G=None, h=None, lb=None, ub=None, device=None, n=None):
        """Build from host arrays: P (B,n,n), q (B,n); A (me,n)|(B,me,n), b; G, h; lb, ub
        ((n,) shared or (B,n)).  Equality rows are stored first (lg == ug).  P = None (with
        ``n``): constraints only -- one problem, P left None and q zero, for callers that set
        the objective on the device afterwards (no n x n host array or upload)."""
        if P is None:
            B, n = 1, int(n)
        else:
            P = np.asarray(P, dtype=np.float64)
            if P.ndim == 2:
                P = P[None]
            B, n, _ = P.shape
            q = np.asarray(q, dtype=np.float64).reshape(B, n)

        def per(M, rows):
            if M is None:
                return None
            M = np.asarray(M, dtype=np.float64)
            if M.ndim == 1 and rows is not None:
                M = M.reshape(rows)
            return M

        A = None if A is None else np.asarray(A, dtype=np.float64)
        G = None if G is None else np.asarray(G, dtype=np.float64)
        if A is not None and A.ndim == 1:
            A = A.reshape(1, n)
        if G is not None and G.ndim == 1:
            G = G.reshape(1, n)
        me = 0 if A is None else A.shape[-2]
        mi = 0 if G is None else G.shape[-2]
        shared = (A is None or A.ndim == 2) and (G is None or G.ndim == 2)
        b_ = None if b is None else np.asarray(b, dtype=np.float64)
        h_ = None if h is None else np.asarray(h, dtype=np.float64)
        if shared and b_ is not None and b_.size != me:
            shared = False
        if shared and h_ is not None and h_.size != mi:
            shared = False
        lb_ = None if lb is None else np.asarray(lb, dtype=np.float64)
        ub_ = None if ub is None else np.asarray(ub, dtype=np.float64)
        if shared and ((lb_ is not None and lb_.ndim == 2) or (ub_ is not None and ub_.ndim == 2)):
            shared = False
        has_box = lb_ is not None or ub_ is not None
        self = cls(n, B, me + mi, device=device, shared_constraints=shared, has_box=has_box,
                   P=None if P is not None else torch.empty(0, dtype=F64))
        nc = 1 if shared else B
        ld = self.ld
        Cg = np.zeros((nc, max(me + mi, 1), ld))
        lg = np.full((nc, max(me + mi, 1)), -np.inf)
        ug = np.full((nc, max(me + mi, 1)), np.inf)
        if me:
            Ab = np.broadcast_to(A, (nc, me, n)) if A.ndim == 2 else A
            bb = np.broadcast_to(b_.reshape(-1, me) if b_ is not None else 0.0, (nc, me))
            Cg[:, :me, :n] = Ab
            lg[:, :me] = bb
            ug[:, :me] = bb
        if mi:
            Gb = np.broadcast_to(G, (nc, mi, n)) if G.ndim == 2 else G
            hb = np.broadcast_to(h_.reshape(-1, mi), (nc, mi))
            Cg[:, me:me + mi, :n] = Gb
            ug[:, me:me + mi] = hb
        dev = self.device
        if P is None:
            self.P = None
        else:
            Pp = np.zeros((B, ld, ld))
            Pp[:, :n, :n] = P
            self.P = torch.from_numpy(Pp).to(dev)
            qp = np.zeros((B, ld))
            qp[:, :n] = q
            self.q = torch.from_numpy(qp).to(dev)
        self.Cg = torch.from_numpy(Cg).to(dev)
        self.lg = torch.from_numpy(lg).to(dev)
        self.ug = torch.from_numpy(ug).to(dev)
        if has_box:
            lo = np.full((nc, ld), -np.inf)
            up = np.full((nc, ld), np.inf)
            lo[:, n:] = 0.0
            up[:, n:] = 0.0
            if lb_ is not None:
                lo[:, :n] = np.broadcast_to(lb_, (nc, n)) if lb_.ndim == 1 else lb_
            if ub_ is not None:
                up[:, :n] = np.broadcast_to(ub_, (nc, n)) if ub_.ndim == 1 else ub_
            self.lb = torch.from_numpy(lo).to(dev)
            self.ub = torch.from_numpy(up).to(dev)
        self.me, self.mi = me, mi
        return self


LR_POLISH_LDK = 256      # first compact polish scratch of the window path (free set <= 256)


class Workspace:
    """Solver state for a QPBatch (all device memory; nothing persistent in the library).

    ``dense`` (K2/K3/K4 on P itself): K / Dt are the n x n KKT inverse and polish scratch.
    Otherwise (the window path) they are only the compact ldk x ldk polish scratch of
    pq_polish_w_batched, ldk = ``kcap`` (default min(ld, LR_POLISH_LDK))."""

    def __init__(self, qb: QPBatch, dense: bool = True, kcap: int | None = None):
        B, ld, dev = qb.batch, qb.ld, qb.device
        self.B, self.device = B, dev
        self.mg_pad = qb.mg_pad
        self.m_ld = qb.mg_pad + ld
        self.ldk = ld if dense else min(ld, 1024, round_up(kcap or LR_POLISH_LDK, 64))
        kd = self.ldk
        self.K = torch.empty((B, kd, kd), dtype=F64, device=dev)
        self.Dt = torch.empty((B, kd // 64, 64, 64), dtype=F64, device=dev)
        self._lr = None
        self.x = torch.zeros((B, ld), dtype=F64, device=dev)
        self.Px = torch.zeros((B, ld), dtype=F64, device=dev)
        self.z = torch.zeros((B, self.m_ld), dtype=F64, device=dev)
        self.y = torch.zeros((B, self.m_ld), dtype=F64, device=dev)
        self.rho = torch.zeros(B, dtype=F64, device=dev)
        self.iters = torch.zeros(B, dtype=torch.int32, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.info = torch.zeros(B, dtype=torch.int32, device=dev)
        self.out = torch.zeros((B, _lib.PQ_OUT_FIELDS), dtype=F64, device=dev)
        self.work_stride = _lib.work_doubles(ld, qb.mg_pad)
        self.work = torch.zeros((B, self.work_stride), dtype=F64, device=dev)
        # set by every solve_lowrank for its callers: the group capacitance's plan and the SweepPlan the
        # ADMM ran on, the band Gram's (rows, width), the dates the grouped polish handed back
        self.gcap_groups = self.sweep_admm = self.band_shape = self.pg_fallback = None
        # built on first use and kept (captured graphs point to them): the grouped polish's record and
        # pass scratch, the sync-free flag, the GroupCap of the ADMM and of the wide polish rounds
        self._pg_rec = self._pg_pass = self._sf_flag = self._gcap = self._pgw = None

    def pg_record(self):
        """Per-problem record of the grouped polish pipeline (PQ_PG_RECORD doubles each)."""
        if self._pg_rec is None:
            self._pg_rec = torch.zeros((self.B, _lib.PQ_PG_RECORD), dtype=F64, device=self.device)
        return self._pg_rec

    def lr_buffers(self, k_ld: int):
        """Capacitance matrices M, their inverses and factor scratch (low-rank path)."""
        if self._lr is None or self._lr["k_ld"] != k_ld:
            self._lr = dict(_matrix_stack(self.B, k_ld, self.device), k_ld=k_ld)
        return self._lr

    def c_struct(self, K=None, Dt=None) -> _lib.PQState:
        """The state struct; ``K`` / ``Dt``: another matrix stack and factor scratch in place of the workspace's."""
        K, Dt = self.K if K is None else K, self.Dt if Dt is None else Dt
        return _lib.PQState(
            K=K.data_ptr(), K_stride=K.stride(0), Dt=Dt.data_ptr(), Dt_stride=Dt.stride(0),
            x=self.x.data_ptr(), Px=self.Px.data_ptr(),
            z=self.z.data_ptr(), y=self.y.data_ptr(),
            m_ld=self.m_ld, mg_pad=self.mg_pad,
            rho=self.rho.data_ptr(),
            iters=self.iters.data_ptr(), status=self.status.data_ptr(), info=self.info.data_ptr(),
            out=self.out.data_ptr(),
            work=self.work.data_ptr(), work_stride=self.work_stride)


@dataclass
class BatchResult:
    x: torch.Tensor          # (B, n) weights (device)
    y: torch.Tensor          # (B, mg) multipliers of the general rows (equalities first)
    z_box: torch.Tensor      # (B, n)
    status: torch.Tensor     # (B,) int32
    iters: torch.Tensor      # (B,) int32
    # (B, PQ_OUT_FIELDS): the certificate of the returned point, written by the polish kernel that
    # scored it -- OBJ, PRIM, DUAL, GAP (qpsolvers' definitions, of exactly the x, y, z_box above),
    # RHO, NFREE, ROUNDS.  With the polish off (Settings.polish = 0 / polish=False) nothing scores
    # the ADMM point and OBJ, PRIM, DUAL, GAP are NaN: an unscored point is not a certified one
    out: torch.Tensor
    refactors: int = 0
    admm_launches: int = 0
    polish_fallbacks: int = 0   # dates the grouped polish handed to the per-date kernel
    capacitance: str = ""    # window path: "band" (pq_lr_capacitance_band), "group", "eig" or "direct"

    @property
    def obj(self):
        return self.out[:, _lib.PQ_OUT_OBJ]

    @property
    def found(self):
        return (self.status == _lib.PQ_SOLVED) | (self.status == _lib.PQ_SOLVED_INACCURATE)


class StageGraphs:
    """HIP graphs of the stages of a solve that is repeated on the same buffers (a backtest
    re-solved every step, the bench workloads): the first time a stage runs its launches are
    captured into a graph (torch.cuda.CUDAGraph over the caller's stream: the library's
    kernels, the side-stream forks / joins of the polish and the torch glue), every later
    time the graph is replayed -- one launch per stage instead of dozens, no host work
    between them.  Stages are keyed by name and occurrence within one solve (``begin``).

    Only sync-free stages may be captured (solve_lowrank(sync_free=True) is); kernel
    arguments -- device pointers and settings -- are frozen at capture, so the owner must
    keep the same problem, window and workspace objects alive and in place."""

    def __init__(self):
        self.graphs = {}
        self.pool = None
        self._seen = {}
        self._warm = set()
        self.replays = 0   # replays of a graph captured by an earlier step (tests, diagnostics)

    def begin(self):
        self._seen = {}

    def run(self, name, fn):
        """First call of a stage: eager (it fills the host-side caches -- plans, uniformity
        checks -- whose first evaluation synchronises); second: capture + replay; then replay."""
        k = self._seen.get(name, 0)
        self._seen[name] = k + 1
        key = (name, k)
        hit = self.graphs.get(key)
        if hit is not None:
            self.replays += 1
        if hit is None:
            if key not in self._warm:
                self._warm.add(key)
                return fn()
            # captured on the caller's (non-default) stream itself: the solve passes that
            # stream to the library explicitly, so it must be the capturing one
            cur = torch.cuda.current_stream()
            if cur == torch.cuda.default_stream(cur.device):
                raise RuntimeError("StageGraphs: run the solve on a non-default stream (torch.cuda.stream(...))")
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self.pool, stream=cur):
                r = fn()
            self.pool = g.pool()
            hit = self.graphs[key] = (g, r)
        hit[0].replay()
        return hit[1]


class _Timeline:
    """Optional per-launch HIP event pairs on the launch stream (no host syncs); with
    ``graphs`` (StageGraphs) each stage is captured once and replayed afterwards (the events
    then bracket the graph launch)."""

    def __init__(self, sink, graphs: "StageGraphs | None" = None):
        self.sink = sink
        self.graphs = graphs

    def __call__(self, name, fn):
        run = (lambda: self.graphs.run(name, fn)) if self.graphs is not None else fn
        if self.sink is None:
            return run()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        r = run()
        e1.record()
        self.sink.append((name, e0, e1))
        return r


def solve(qb: QPBatch, settings: Settings | None = None, ws: Workspace | None = None,
          max_rounds: int = 64, events: list | None = None) -> BatchResult:
    """Solve every QP of the batch on the current device/stream (K2 -> K3 [-> K2 -> K3 ...] -> K4).

    ``events``: if a list is given, (kernel name, start, end) torch.cuda.Event triples are
    appended for every launch (recorded on the launch stream)."""
    tl = _Timeline(events)
    lib = _lib.load()
    settings = settings or Settings()
    s = settings.to_c()
    ws = ws or Workspace(qb)
    pb = qb.c_struct()
    st = ws.c_struct()
    strm = _stream()
    P_, S_, SS = ctypes.byref(pb), ctypes.byref(st), ctypes.byref(s)
    s_init = _init_settings(settings)
    _lib.check(lib.pq_init_state(P_, S_, None, 0, ctypes.byref(s_init), strm), "pq_init_state")
    _rho_floor_q(qb, ws, settings, in_kernel=s_init.rho0_qrel > 0)
    _lib.check(tl("factor", lambda: lib.pq_factor_batched(P_, S_, None, 0, SS, 1, strm)),
               "pq_factor_batched")
    cnt = {"refactors": 0, "launches": 0}

    def admm_rounds(idx, nidx, SSx):
        for _ in range(max_rounds):
            _lib.check(tl("admm", lambda: lib.pq_admm_batched(P_, S_, _ptr(idx), nidx, SSx,
                                                              int(s.max_iter), strm)),
                       "pq_admm_batched")
            cnt["launches"] += 1
            need = torch.nonzero(ws.status == _lib.PQ_NEED_REFACTOR).flatten().to(torch.int32)
            k = int(need.numel())   # host sync: small status vector
            if k == 0:
                break
            idx, nidx = need.contiguous(), k
            _lib.check(tl("factor", lambda: lib.pq_factor_batched(P_, S_, _ptr(idx), nidx, SSx, 1, strm)),
                       "pq_factor_batched")
            cnt["refactors"] += k

    admm_rounds(None, 0, SS)
    if s.polish:
        _lib.check(tl("polish", lambda: lib.pq_polish_batched(P_, S_, None, 0, SS, strm)),
                   "pq_polish_batched")
        rp = _repolish_set(ws, settings)
        if rp is not None:      # polish rejected: polish again with more refinement steps
            pidx, pn, s3 = rp
            _lib.check(tl("polish", lambda: lib.pq_polish_batched(P_, S_, _ptr(pidx), pn, ctypes.byref(s3), strm)),
                       "pq_polish_batched (refine)")
        retry = _retry_set(ws, settings)
        if retry is not None:   # polish rejected: resume ADMM to eps_retry, polish again
            idx, nidx, s2 = retry
            # the polish used K as scratch: restore K^-1 (current rho) before resuming
            _lib.check(tl("factor", lambda: lib.pq_factor_batched(P_, S_, _ptr(idx), nidx, SS, 1, strm)),
                       "pq_factor_batched (retry)")
            admm_rounds(idx, nidx, ctypes.byref(s2))
            _lib.check(tl("polish", lambda: lib.pq_polish_batched(P_, S_, _ptr(idx), nidx, SS, strm)),
                       "pq_polish_batched (retry)")
    return _batch_result(qb, ws, refactors=cnt["refactors"], admm_launches=cnt["launches"])


def _batch_result(qb: "QPBatch", ws: "Workspace", **counts) -> BatchResult:
    n, mg = qb.n, qb.mg
    return BatchResult(x=ws.x[:, :n], y=ws.y[:, :mg], z_box=ws.y[:, ws.mg_pad:ws.mg_pad + n],
                       status=ws.status, iters=ws.iters, out=ws.out, **counts)


def _init_settings(settings: Settings) -> _lib.PQSettings:
    """The settings of the init call of solve / solve_lowrank: with pq_settings.rho0_qrel, so that
    k_init_state applies the |q| floor of the initial rho (every other call leaves the field at 0)."""
    return settings.to_c(rho0_qrel=0.0 if RHO_FLOOR_HOST else max(float(settings.rho0_qrel), 0.0))


def _rho_floor_q(qb: "QPBatch", ws: "Workspace", settings: Settings, in_kernel: bool = False):
    """Initial rho >= rho0_qrel * max|q| per problem (both paths, before the first factor).
    ``in_kernel``: the init call carried pq_settings.rho0_qrel, so k_init_state has stored the
    same values already and nothing is launched here."""
    if settings.rho0_qrel > 0 and not in_kernel:
        qinf = qb.q[:, :qb.n].abs().amax(1)
        torch.clamp(torch.maximum(ws.rho, settings.rho0_qrel * qinf), settings.rho_min, settings.rho_max,
                    out=ws.rho)


def sf_flag_torch(rec: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    """The sync-free flag from the grouped polish's record and the status vector: any date pending, handed
    back, rejected or unsolved, or an ADMM refactor requested (what k_pg_post notes at PQ_PG_SFLAG)."""
    st_pg = rec[:, _lib.PQ_PG_STATE]
    return ((st_pg == _lib.PQ_PG_PENDING) | (st_pg == _lib.PQ_PG_FALLBACK) |
            (status == _lib.PQ_NEED_REFACTOR) | (status == _lib.PQ_SOLVED_INACCURATE) |
            (status == _lib.PQ_UNSOLVED)).any()


def _repolish_set(ws: "Workspace", settings: Settings):
    """Problems whose polish was rejected: set them back to SOLVED (their ADMM point is
    untouched by a rejected polish) and return (idx, n, settings with refine_iters =
    refine_retry) for a second polish, or None (host sync: status)."""
    if settings.refine_retry <= settings.refine_iters:
        return None
    bad = torch.nonzero(ws.status == _lib.PQ_SOLVED_INACCURATE).flatten().to(torch.int32)
    m = int(bad.numel())
    if m == 0:
        return None
    ws.status[bad.long()] = _lib.PQ_SOLVED
    return bad.contiguous(), m, settings.to_c(refine_iters=settings.refine_retry)


def _retry_set(ws: "Workspace", settings: Settings):
    """Problems whose polish was rejected at the loose ADMM eps: reset them to UNSOLVED
    and return (idx, n, settings with eps = eps_retry), or None (host sync: status)."""
    bad = torch.nonzero(ws.status == _lib.PQ_SOLVED_INACCURATE).flatten().to(torch.int32)
    m = int(bad.numel())
    if m == 0 or settings.eps_retry <= 0 or settings.eps_retry >= min(settings.eps_abs, settings.eps_rel):
        return None
    ws.status[bad.long()] = _lib.PQ_UNSOLVED
    return bad.contiguous(), m, settings.to_c(eps_abs=settings.eps_retry, eps_rel=settings.eps_retry)


def _window_span(rows, tlen):
    """(r0, nrows, W) of a device row table: the panel rows the windows touch and the widest
    window span (one host read)."""
    t = tlen.to(torch.int64)
    first = rows[:, 0].to(torch.int64)
    last = rows.gather(1, (t - 1).clamp(min=0)[:, None]).flatten().to(torch.int64)
    v = torch.stack([first.min(), last.max(), (last - first + 1).max()]).cpu().tolist()
    return int(v[0]), int(v[1] - v[0] + 1), int(v[2])


class LowRank:
    """Device description of P_eff = p_scale w_scale Xc'Xc + p_diag I through the date
    windows (pq_lowrank): nothing n x n is formed.  ``mu`` None = uncentred Gram
    (LeastSquares).  ``dg`` = diag(Xc'Xc) per date (pq_window_sumsq; computed here when
    not given -- call refresh() after the window means change in place)."""

    def __init__(self, panel, rows, tlen, mu=None, w_scale=None, dg=None):
        self.panel, self.rows, self.tlen, self.mu, self.w_scale = panel, rows, tlen, mu, w_scale
        self.tmax = int(rows.shape[1])
        self.dg = dg if dg is not None else panel.window_sumsq(rows, tlen, mu)
        self._span = None

    def refresh(self):
        self.panel.window_sumsq(self.rows, self.tlen, self.mu, out=self.dg)
        return self

    def span(self):
        """(r0, nrows, W): the panel rows the windows touch and the widest window span."""
        if self._span is None:
            self._span = _window_span(self.rows, self.tlen)
        return self._span

    def c_struct(self) -> _lib.PQLowRank:
        return _lib.PQLowRank(panel=self.panel.R.data_ptr(), ldp=self.panel.R.stride(0),
                              rows=self.rows.data_ptr(), tlen=self.tlen.data_ptr(), tmax=self.tmax,
                              mu=None if self.mu is None else self.mu.data_ptr(),
                              mu_stride=0 if self.mu is None else self.mu.stride(0),
                              w_scale=None if self.w_scale is None else self.w_scale.data_ptr(),
                              dg=self.dg.data_ptr(), dg_stride=self.dg.stride(0))


class EigCap:
    """One symmetric eigendecomposition per DATE of the centred window Gram Xc Xc' (T x T),
    shared by every problem of that date (pq_eigcap_form): the risk aversions of the sweep
    (P = 2 lam Sigma_d, src/optimization.py:168-174) differ only in the scale of P and in
    rho, and each capacitance inverse M_b^-1 is formed from the date's eigenvectors for the
    problem's own scale and rho -- no per-problem factorisation, and an adaptive-rho change
    is a re-form.  The Gram and the border W = Xc Cg' come from the hand-written window Gram
    kernel (pq_lr_capacitance with D = I, unit row weights); the eigendecomposition itself
    is rocSOLVER's (torch.linalg.eigh, ``backend`` 'rocsolver', the default) or the hand-written
    block-Jacobi solver (jacobi.hip, helper_functions.sym_eig, 'jacobi'), once per date.
    Measured for the 64 window Grams of config 5 (profiles/r03k_exp_eigh.log): syevd 10.4 ms,
    the block-Jacobi kernels 64.5 ms (eigenvalues to 1.2e-12) -- the Jacobi form serves the
    nearestPD repair, whose matrices need no ordering.  (Not few sweeps: a rank-deficient
    covariance takes more than a dense matrix of its size, 24 of the 30 allowed at n = 1000,
    T = 252)

    rows / tlen / mu: per-date device tensors (every tlen == tmax); pdate: date of each
    problem (int32, device); Cg: the shared general rows (qb.Cg, mg <= 4)."""

    MG = 4

    def __init__(self, panel, rows, tlen, mu, qb: "QPBatch", pdate, k_ld: int, backend: str = "rocsolver"):
        lib = _lib.load()
        nd, tmax = int(rows.shape[0]), int(rows.shape[1])
        mg, n, dev = qb.mg, qb.n, qb.device
        if mg > self.MG or not qb.shared:
            raise _lib.PorquaHipError("EigCap: shared general rows, at most 4")
        if not bool((tlen == tmax).all().item()):
            raise _lib.PorquaHipError("EigCap: every window must have tmax rows")
        self.k_ld, self.nd, self.tmax = int(k_ld), nd, tmax
        self.pdate = pdate.to(torch.int32).contiguous()
        lgf = torch.full((max(mg, 1),), -np.inf, dtype=F64, device=dev)
        ugf = torch.full((max(mg, 1),), np.inf, dtype=F64, device=dev)
        one = torch.ones(nd, dtype=F64, device=dev)
        pb = _lib.PQProblem(n=n, ld=qb.ld, batch=nd, mg=mg, P=None, P_stride=0, p_scale=None, p_diag=None,
                            q=qb.q.data_ptr(), q_stride=0, Cg=qb.Cg.data_ptr(), Cg_stride=0,
                            lg=lgf.data_ptr(), ug=ugf.data_ptr(), g_stride=0, lb=None, ub=None, box_stride=0)
        lr = _lib.PQLowRank(panel=panel.R.data_ptr(), ldp=panel.R.stride(0), rows=rows.data_ptr(),
                            tlen=tlen.data_ptr(), tmax=tmax, mu=mu.data_ptr(), mu_stride=mu.stride(0),
                            w_scale=None, dg=None, dg_stride=0)
        st = _lib.PQState(rho=one.data_ptr())
        s = Settings(sigma=1.0, rho_min=1.0).to_c()   # D = I, unit weight on the Cg rows: M = I + U U'
        M = torch.zeros((nd, k_ld, k_ld), dtype=F64, device=dev)
        _lib.check(lib.pq_lr_capacitance(ctypes.byref(lr), ctypes.byref(pb), ctypes.byref(st), None, 0,
                                         ctypes.byref(s), M.data_ptr(), k_ld, k_ld * k_ld, _stream()),
                   "pq_lr_capacitance (window Gram)")
        T = tmax
        Mt = M[:, :T, :T]
        G = torch.tril(Mt) + torch.tril(Mt, -1).mT - torch.eye(T, dtype=F64, device=dev)
        if backend == "jacobi":   # zero padding to a multiple of 64: its pairs never rotate
            from .helper_functions import sym_eig
            ldj = round_up(T, 64)
            Gp = torch.zeros((nd, ldj, ldj), dtype=F64, device=dev)
            Gp[:, :T, :T] = G
            evj, Vj = sym_eig(Gp, T)
            ev, V = evj[:, :T], Vj[:, :T, :T]
        elif backend == "rocsolver":
            ev, V = torch.linalg.eigh(G)
        else:
            raise ValueError("EigCap: backend must be 'jacobi' or 'rocsolver'")
        self.V = torch.zeros((nd, k_ld, k_ld), dtype=F64, device=dev)
        self.V[:, :T, :T] = V
        self.evals = torch.zeros((nd, k_ld), dtype=F64, device=dev)
        self.evals[:, :T] = ev
        self.What = torch.zeros((nd, k_ld, self.MG), dtype=F64, device=dev)
        if mg:
            W = M[:, T:T + mg, :T].mT                      # Xc Cg' (rows T.. of the lower triangle)
            self.What[:, :T, :mg] = V.mT @ W
            C = qb.Cg[0, :mg, :n]
            self.cc = (C @ C.T).contiguous()
        else:
            self.cc = torch.zeros((1, 1), dtype=F64, device=dev)
        self.scratch = torch.empty((qb.batch, 2 * self.MG * k_ld), dtype=F64, device=dev)

    def form(self, lrs, pbs, sts, ss, Minv, idx, nidx, strm):
        """M_b^-1 of problems idx[0..nidx) (None: all) into Minv (B, k_ld, k_ld)."""
        lib = _lib.load()
        k = self.k_ld
        _lib.check(lib.pq_eigcap_form(lrs, pbs, sts, ss, self.pdate.data_ptr(), self.V.data_ptr(),
                                      self.evals.data_ptr(), self.What.data_ptr(), self.cc.data_ptr(), k,
                                      _ptr(idx), nidx, Minv.data_ptr(), k * k, self.scratch.data_ptr(), strm),
                   "pq_eigcap_form")


def lowrank_shape_ok(n: int, tmax: int, mg: int) -> bool:
    """The Woodbury path applies (and pays): T + mg < n, k <= 512, and the window-form polish
    can run (even panel stride n, tmax <= 1024) so nothing needs the dense upper triangle."""
    k_ld = round_up(tmax + mg, 64)
    return (k_ld <= 512 and (k_ld + 127) // 128 <= (n + 127) // 128 and tmax + mg < n
            and n % 2 == 0 and tmax <= 1024 and mg <= 64)


def lowrank_applicable(qb: QPBatch, lr: LowRank) -> bool:
    return lowrank_shape_ok(qb.n, lr.tmax, qb.mg) and lr.panel.R.stride(0) % 2 == 0


def grouped_applicable(qb: QPBatch, lr: LowRank, groups: "GroupPlan | None", ws: "Workspace") -> bool:
    k_ld = round_up(lr.tmax + qb.mg, 64)
    return (groups is not None and groups.ok and qb.n % 2 == 0 and lr.panel.R.stride(0) % 2 == 0
            and qb.mg <= 32 and k_ld <= 384 and ws.work_stride >= 3 * qb.ld)


def _sparse_columns(qb: QPBatch, nz_limit: int = 4):
    """Column-sparse form of shared general rows (more than 4 rows, at most ``nz_limit``
    nonzeros per column: the budget row plus 0/1 group memberships, Constraints.add_linear
    for sector caps) for pq_admm_lr_grouped: (row ids int32 [ld, nzmax] -1 padded, values,
    nzmax), or (None, None, 0) when the rows are few or dense."""
    if not qb.shared or qb.mg <= 4:
        return None, None, 0
    C = qb.Cg[0, :qb.mg, :]
    nzc = (C != 0).sum(0)
    nzmax = int(nzc.max().item())
    if nzmax == 0 or nzmax > nz_limit:
        return None, None, 0
    order = torch.argsort((C == 0).to(torch.int8), dim=0, stable=True)[:nzmax]   # nonzero rows first
    vals = torch.gather(C, 0, order)
    rows = torch.where(vals != 0, order, torch.full_like(order, -1)).to(torch.int32)
    return rows.T.contiguous(), vals.T.contiguous(), nzmax


def _tkey(*ts):
    """Cache key of tensors (None allowed): storage, shape and in-place version counter, so
    it changes when a tensor is replaced or modified in place."""
    return tuple(None if t is None else (t.data_ptr(), tuple(t.shape), t._version) for t in ts)


def _cached(owner, name: str, key, fn, keep=()):
    """fn() cached on ``owner`` under ``name`` while ``key`` is unchanged (host-side checks
    with device syncs and constant tables are then paid once per batch, not per solve).

    ``keep``: the objects whose identity the key encodes (``id()``s, tensor data pointers).
    The cache entry holds strong references to them, so while the entry lives no other
    object can reuse those ids or the caching allocator those addresses, and a key match
    means the same objects (in-place changes bump ``_version``, which the key includes)."""
    hit = getattr(owner, name, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    val = fn()
    setattr(owner, name, (key, val, tuple(keep)))
    return val


def _uniform_box(qb: QPBatch) -> bool:
    """Every box row of every problem gets the same ADMM rho (pq_lr_capacitance_band)."""
    if qb.lb is None:
        return True
    n = qb.n

    def check():
        lo, up = qb.lb[:, :n], qb.ub[:, :n]
        cls = torch.where(torch.isinf(lo) & torch.isinf(up), 1, torch.where(lo == up, 2, 0))
        return bool((cls == cls[:, :1]).all().item()) and (qb.lb.shape[0] == 1 or
                                                          bool((cls[:, 0] == cls[0, 0]).all().item()))
    return _cached(qb, "_c_ubox", _tkey(qb.lb, qb.ub), check, keep=(qb.lb, qb.ub))


def _band_applies(qb: QPBatch, lr: LowRank) -> bool:
    """Shared constraints, tmax <= 1024 and one ADMM rho for every box row (a cached device check)."""
    return qb.shared and lr.tmax <= 1024 and _uniform_box(qb)


def _band_setup(qb: QPBatch, lr: LowRank, strm, w_min: int = 0):
    """Band Gram of the panel rows + PC / CC tables for pq_lr_capacitance_band, or None when
    the band form does not apply (per-problem constraints, non-uniform box rho, tmax > 1024).
    ``w_min``: band width at least this (the group capacitance needs the widest union span)."""
    if not _band_applies(qb, lr):
        return None
    lib = _lib.load()
    r0, nrows, W = lr.span()
    W = min(max(W, int(w_min)), nrows)
    dev, n, mg = qb.device, qb.n, qb.mg
    ldo = round_up(W, 2)
    band, pc = _cached(lr, "_c_bandbuf", (nrows, ldo, mg),
                       lambda: (torch.empty((nrows, ldo), dtype=F64, device=dev),
                                torch.empty((nrows, max(mg, 1)), dtype=F64, device=dev)))
    R = lr.panel.R
    _lib.check(lib.pq_lr_band_gram(R.data_ptr(), R.stride(0), n, r0, nrows, W, band.data_ptr(), ldo,
                                   qb.Cg.data_ptr(), mg, qb.ld, pc.data_ptr(), pc.stride(0), strm),
               "pq_lr_band_gram")
    def cgram():
        C = qb.Cg[0, :mg, :n]
        return (C @ C.T).contiguous() if mg else torch.zeros((1, 1), dtype=F64, device=dev)
    cc = _cached(qb, "_c_cc", _tkey(qb.Cg), cgram, keep=(qb.Cg,))
    # "cap" / "admm": the argument runs the capacitance kernels / the fused ADMM kernels take
    return {"band": band, "ldo": ldo, "r0": r0, "pc": pc, "cc": cc, "W": W, "nrows": nrows,
            "cap": (band.data_ptr(), ldo, r0, pc.data_ptr(), pc.stride(0)),
            "admm": (pc.data_ptr(), pc.stride(0), r0, cc.data_ptr())}


SHRINKAGE_KINDS = {"ledoit_wolf": 0, "oas": 1}


def shrinkage_intensity(panel: "Panel", rows, tlen, kind: str = "ledoit_wolf", centred: bool = True):
    """Data-driven shrinkage intensity of every window towards mean(diag S) I (Ledoit-Wolf
    2004 or OAS, Chen et al. 2010: sklearn's ledoit_wolf_shrinkage / oas) -> (delta (B,),
    stats (B, 4) = a, f, g, delta), device tensors.  ``rows`` / ``tlen``: the device row table
    (Panel.rows_to_device), complete windows.  The band Gram of the rows the windows touch
    (pq_lr_band_gram, W = the widest span) is rebuilt on every call -- the panel may have
    changed -- into a buffer kept with the panel; pq_shrink_stats_band then reads each date's
    T x T window Gram from it.  Synchronises (the kernel's row-table check is read back)."""
    if kind not in SHRINKAGE_KINDS:
        raise ValueError(f"shrinkage_intensity: unknown kind {kind!r} (expected one of {sorted(SHRINKAGE_KINDS)})")
    lib = _lib.load()
    B, tmax = int(rows.shape[0]), int(rows.shape[1])
    dev = panel.device
    stats = torch.empty((B, 4), dtype=F64, device=dev)
    if B == 0:
        return stats[:, 3].contiguous(), stats
    r0, nrows, W = _cached(panel, "_c_shrink_span", _tkey(rows, tlen), lambda: _window_span(rows, tlen),
                           keep=(rows, tlen))
    if r0 < 0 or r0 + nrows > panel.D or W < 1:
        raise ValueError("shrinkage_intensity: the row table points outside the panel")
    ldo = round_up(W, 2)
    band = _cached(panel, "_c_shrink_band", (nrows, ldo),
                   lambda: torch.empty((nrows, ldo), dtype=F64, device=dev))
    R = panel.R
    strm = _stream()
    _lib.check(lib.pq_lr_band_gram(R.data_ptr(), R.stride(0), panel.n, r0, nrows, W, band.data_ptr(), ldo,
                                   None, 0, 0, None, 0, strm), "pq_lr_band_gram")
    rows = rows.contiguous()   # row pitch tmax, as every window entry point reads the table
    _lib.check(lib.pq_shrink_stats_band(band.data_ptr(), ldo, r0, nrows, W, rows.data_ptr(), tmax,
                                        tlen.data_ptr(), tmax, B, panel.n, int(bool(centred)),
                                        SHRINKAGE_KINDS[kind], stats.data_ptr(), strm), "pq_shrink_stats_band")
    return stats[:, 3].contiguous(), stats


def _group_uniform(qb: QPBatch, lr: "LowRank", groups: "GroupPlan") -> bool:
    """The dates of every group share c = p_scale w_scale and p_diag, so one capacitance per
    group serves them all (a device fact, checked once per plan and batch)."""
    B, dev = qb.batch, qb.device

    def uniform():
        one = torch.ones(B, dtype=F64, device=dev)
        c = (qb.p_scale if qb.p_scale is not None else one) * (lr.w_scale if lr.w_scale is not None else one)
        pd = qb.p_diag if qb.p_diag is not None else torch.zeros(B, dtype=F64, device=dev)
        first = groups.gdates[:-1].long()[groups.gidx.long()]
        return bool(((c == c[first]) & (pd == pd[first])).all().item())
    return _cached(groups, "_c_uniform", (B,) + _tkey(qb.p_scale, lr.w_scale, qb.p_diag), uniform,
                   keep=(qb.p_scale, lr.w_scale, qb.p_diag))


def _matrix_stack(count: int, k_ld: int, dev, nstatus: int | None = None) -> dict:
    """``count`` k x k matrices M, their inverses Minv, the factor kernels' scratch and per-matrix outputs."""
    def ints(m):
        return torch.zeros(m, dtype=torch.int32, device=dev)
    return {"M": torch.empty((count, k_ld, k_ld), dtype=F64, device=dev),
            "Minv": torch.empty((count, k_ld, k_ld), dtype=F64, device=dev),
            "Dt": torch.empty((count, k_ld // 64, 64, 64), dtype=F64, device=dev),
            "iters": ints(count), "status": ints(nstatus or count), "info": ints(count)}


def _factor_view(qb: QPBatch, ws: "Workspace", buf: dict, n: int, rho: torch.Tensor):
    """(PQProblem, PQState) that present the k x k matrices buf["M"] to the factor kernels as "problems" of
    size ``n`` (the padded tail of each is the identity: its pivot steps are skipped); inverses to buf["Minv"]."""
    k_ld = buf["M"].shape[1]
    pb = _lib.PQProblem(n=n, ld=k_ld, batch=buf["M"].shape[0], mg=0, P=buf["M"].data_ptr(), P_stride=k_ld * k_ld,
                        q=qb.q.data_ptr(), q_stride=qb.q.stride(0), Cg=qb.Cg.data_ptr(), lg=qb.lg.data_ptr(),
                        ug=qb.ug.data_ptr())
    st = ws.c_struct(buf["Minv"], buf["Dt"])
    st.rho, st.iters, st.status, st.info = (t.data_ptr() for t in (rho, buf["iters"], buf["status"], buf["info"]))
    return pb, st


class GroupCap:
    """Group capacitance (admm_gcap.hip): one matrix M_U per date group plus every date's low-rank
    correction a_b, q_b, H_b^-1 -- the buffers, the PQGcap struct and the factor's view of the M_U stack.
    ``mg`` general rows sit inside the capacitance (the ADMM's; the wide polish rounds' has none).
    ``old``: the workspace's previous GroupCap of this use; its buffers are taken over while the shapes stay
    (the workspace keeps the object, and with it the device memory captured graphs point to, alive)."""

    def __init__(self, qb: QPBatch, ws: "Workspace", groups: "GroupPlan", old: "GroupCap | None", mg: int,
                 nstatus: int | None = None, gmax: int = 0):
        B, dev, G = qb.batch, qb.device, groups.ngroups
        kmax = groups.ucnt_max + mg
        k_ld, ldh = round_up(kmax, 64), min(64, round_up(groups.corr_max, 8))
        self.key = (B, G, k_ld, ldh)
        if old is not None and old.key == self.key:
            buf = old.buf
        else:
            buf = dict(_matrix_stack(G, k_ld, dev, nstatus), grho=torch.empty(G, dtype=F64, device=dev),
                       aq=torch.empty((B, 2 * k_ld), dtype=F64, device=dev),
                       hinv=torch.empty((B, ldh, ldh), dtype=F64, device=dev))
        self.buf = buf
        self.c = _lib.PQGcap(gdates=groups.gdates.data_ptr(), ngroups=G, urows=groups.urows.data_ptr(),
                             ucnt=groups.ucnt.data_ptr(), uoff=groups.uoff.data_ptr(), umax=groups.umax,
                             gidx=groups.gidx.data_ptr(), grho=buf["grho"].data_ptr(), M=buf["M"].data_ptr(),
                             Minv=buf["Minv"].data_ptr(), k_ld=k_ld, M_stride=k_ld * k_ld,
                             aq=buf["aq"].data_ptr(), aq_stride=2 * k_ld, hinv=buf["hinv"].data_ptr(), ldh=ldh,
                             gmax=gmax)
        # the factor sees each M_U as a k x k "problem" (identity padding beyond its U + mg rows)
        self.pb, self.st = _factor_view(qb, ws, buf, kmax, buf["grho"])

    def build(self, L_, P_, S_, SS, SSf, bd: dict, strm, tag: str = "", large: bool = False,
              reset_status: bool = False):
        """One M_U per group at the current group rho (buf["grho"]), its inverse (settings ``SSf``) and every
        date's a_b, q_b, H_b^-1.  ``reset_status``: the factor and the prepare step share the status buffer."""
        lib, buf = _lib.load(), self.buf
        GC_, PM_, SM_ = ctypes.byref(self.c), ctypes.byref(self.pb), ctypes.byref(self.st)
        _lib.check(lib.pq_gcap_assemble(L_, P_, GC_, SS, *bd["cap"], bd["cc"].data_ptr(), strm),
                   "pq_gcap_assemble" + tag)
        if large:   # (experiment) many workgroups per M_U: K2L, one tile each
            W = buf["W"] = buf["W"] if "W" in buf else torch.empty_like(buf["M"])
            _lib.check(lib.pq_factor_large(PM_, SM_, None, 0, SSf, 2, W.data_ptr(), W.stride(0), strm),
                       "pq_factor_large(M_U)")
        else:
            _lib.check(lib.pq_factor_batched(PM_, SM_, None, 0, SSf, 2, strm), "pq_factor_batched(M_U)" + tag)
        if reset_status:
            buf["status"].zero_()
        _lib.check(lib.pq_gcap_prepare(L_, P_, S_, GC_, SS, None, 0, *bd["cap"], strm), "pq_gcap_prepare" + tag)


def _pg_wide_setup(qb: QPBatch, lr: "LowRank", ws: "Workspace", groups: "GroupPlan", bd: dict, rec: torch.Tensor,
                   settings: Settings, sparse_cols, strm):
    """Group capacitance of the polish matrix K = P + d I for the wide rounds of the grouped
    polish (polish_gw.hip), d = p_diag + delta_g with delta_g the geometric mean of the
    group's dates' delta (settings.delta x problem scale, record field PQ_PG_SC): the ADMM's
    GroupCap with no general rows in the capacitance and a unit box whose rho is delta_g.
    Returns the pq_pg_wide argument (kept alive on ws), or None when the wide form does not apply."""
    B, dev, mg, G = qb.batch, qb.device, qb.mg, groups.ngroups
    nzr, nzv, nzmax = sparse_cols if mg > 4 else (None, None, 0)
    # uncentred windows only (LeastSquares tracking): with a mean column the correction H_b has
    # the entry 1 - (cT/d)(mu'mu - a'q/d), which cancels catastrophically at the polish's small d
    if (lr.mu is not None or bd is None or bd["W"] < groups.span_max or not qb.shared or mg > 24
            or (mg > 4 and nzmax == 0) or groups.ucnt_max + mg > 320 or groups.corr_max > 64
            or not _group_uniform(qb, lr, groups)):
        return None
    gc = ws._pgw = GroupCap(qb, ws, groups, ws._pgw, mg=0, nstatus=max(G, B))
    buf = gc.buf
    if "wscr" not in buf:
        buf.update(wscr=torch.empty((B, _lib.pg_wscr(gc.c.k_ld)), dtype=F64, device=dev),
                   lb=torch.zeros(2, dtype=F64, device=dev), ub=torch.ones(2, dtype=F64, device=dev))
    gi, sizes = groups.device_index()
    ld = torch.log(torch.clamp(settings.delta_wide * rec[:, _lib.PQ_PG_SC], min=1e-300))
    gl = torch.zeros(G, dtype=F64, device=dev).index_add_(0, gi, ld)
    buf["grho"].copy_(torch.exp(gl / sizes))
    # the polish matrix: no general rows in the capacitance, a unit box (rho = delta_g), sigma 0
    pbw = qb.c_struct()
    pbw.mg, pbw.lb, pbw.ub, pbw.box_stride = 0, buf["lb"].data_ptr(), buf["ub"].data_ptr(), 0
    stw = _lib.PQState(status=buf["status"].data_ptr())
    SW = ctypes.byref(Settings(sigma=0.0).to_c())
    gc.build(ctypes.byref(lr.c_struct()), ctypes.byref(pbw), ctypes.byref(stw), SW, SW, bd, strm, tag=" (polish)",
             reset_status=True)
    # a date whose correction H_b is not SPD to rounding, or whose group's M_U failed, keeps the
    # per-date kernel (state FALLBACK before the first round)
    bad = (buf["status"][:B] == _lib.PQ_NON_CONVEX) | (buf["info"][gi] != 0)
    rec[:, _lib.PQ_PG_STATE] = torch.where(bad & (rec[:, _lib.PQ_PG_STATE] == _lib.PQ_PG_PENDING),
                                           float(_lib.PQ_PG_FALLBACK), rec[:, _lib.PQ_PG_STATE])
    pc, ldpc, r0, cc = bd["admm"]
    gc.wide = _lib.PQPgWide(gc=ctypes.pointer(gc.c), pc=pc, ldpc=ldpc, r0=r0, cc=cc, nzr=_ptr(nzr), nzv=_ptr(nzv),
                            nzmax=nzmax, wscr=buf["wscr"].data_ptr(), wscr_stride=buf["wscr"].stride(0),
                            refine_steps=int(settings.refine_wide))
    return gc.wide


def loose_stop_eps(settings: Settings, centred: bool, batch: int, mg: int = 1) -> float:
    """The eps of the loose ADMM stop before the grouped polish (0: none): eps_grouped for
    centred windows, eps_grouped_tracking for uncentred ones; when that is 0,
    eps_grouped_tracking_small (when > 0; default off) for uncentred batches of at most
    small_batch dates, else eps_grouped_tracking_wide for more than 4 general rows (the wide
    form).  eps_grouped = 0 turns every loose stop off."""
    if centred:
        return settings.eps_grouped
    eps = settings.eps_grouped_tracking
    if eps <= 0.0 and settings.eps_grouped > 0.0:
        if batch <= settings.small_batch and settings.eps_grouped_tracking_small > 0.0:
            eps = settings.eps_grouped_tracking_small
        elif mg > 4:
            eps = settings.eps_grouped_tracking_wide
    return eps


@dataclass(frozen=True)
class LowRankRoute:
    """Which kernels one solve_lowrank call runs, decided once by lowrank_route."""
    grouped: bool             # the grouped forms apply (grouped_applicable)
    capacitance: str          # "group", "eig", "band" or "direct" (BatchResult.capacitance)
    admm: str                 # "gcap", "sweep", "grouped-fused", "grouped-unfused" or "per-problem"
    plan: "GroupPlan | None"  # the plan the ADMM runs on (groups, or groups.gcap_plan() for "gcap")
    band: bool                # the band Gram is built
    band_wmin: int            # its minimum width: every union the group capacitances read
    polish: str               # "grouped", "per-date" or "none"
    loose_eps: float          # the loose ADMM stop before the grouped polish (0: off) ...
    loose_min_iter: int       # ... and its pq_settings.min_iter
    sync_free: bool           # the caller's sync_free, honoured
    sparse_cols: tuple = dataclasses.field(default=(None, None, 0), compare=False)   # _sparse_columns


def lowrank_route(qb: QPBatch, lr: LowRank, ws: Workspace, groups: "GroupPlan | None", settings: Settings, *,
                  polish: bool = True, band: bool = True, fuse: bool = True, grouped_polish: bool = True,
                  gcap: bool = True, wide_polish: bool = True, sync_free: bool = False,
                  eig: "EigCap | None" = None, sweep: "SweepPlan | None" = None) -> LowRankRoute:
    """The route of solve_lowrank for these inputs and caller flags.  Two inputs are device facts, read through
    cached checks (one host sync per batch, none in the steady state): _band_applies and _group_uniform."""
    k_ld = round_up(lr.tmax + qb.mg, 64)
    grouped = grouped_applicable(qb, lr, groups, ws)
    sparse_cols = _sparse_columns(qb) if grouped else (None, None, 0)
    # group capacitance: shared rows (none, mg = 0, included), register-resident (mg <= 4) or column-sparse
    # (mg <= 24, <= 4 nonzeros per asset); pass 1 of admm_gcap.hip covers U + mg <= 320 rows
    gcap_try = (gcap and eig is None and grouped and fuse and qb.shared
                and (qb.mg <= 4 or (qb.mg <= 24 and sparse_cols[2] > 0))
                and groups.ucnt_max + qb.mg <= 320 and groups.corr_max <= 64)
    # its own plan: up to 32 dates per group (GroupPlan.gcap_plan), for register-resident general rows and
    # (GCAP32_WIDE) the column-sparse wide form; the polish keeps its 16-date groups (polish_plan)
    gplan = groups
    if gcap_try and (qb.mg <= 4 or GCAP32_WIDE):
        g32 = groups.gcap_plan()
        if g32.ucnt_max + qb.mg <= 320 and g32.corr_max <= 64:
            gplan = g32
    use_band = band and _band_applies(qb, lr)
    # the band must cover every union the capacitances read: the ADMM's groups and the polish's (wide rounds)
    wmin = (max(gplan.span_max, groups.polish_plan().span_max)
            if band and (gcap_try or (grouped and wide_polish)) else 0)
    if gcap_try and use_band and _group_uniform(qb, lr, gplan):
        cap, admm, plan = "group", "gcap", gplan
    else:
        cap = "eig" if eig is not None else ("band" if use_band else "direct")
        fused = use_band and fuse and qb.mg <= 32   # uniform D + shared Cg: the fused form
        plan = groups if grouped else None
        if not grouped:
            admm = "per-problem"
        elif fused and sweep is not None and sweep.applicable(qb, lr, k_ld):
            admm = "sweep"
        else:
            admm = "grouped-fused" if fused else "grouped-unfused"
    pol = "grouped" if (grouped and grouped_polish and ws.ldk >= 64) else "per-date"
    if not (polish and settings.polish):
        pol = "none"
    eps_loose = loose_stop_eps(settings, lr.mu is not None, qb.batch, qb.mg)
    loose = (pol == "grouped" and (admm == "gcap" or (settings.eps_grouped_percap and grouped and eig is None))
             and eps_loose > max(settings.eps_abs, settings.eps_rel))
    return LowRankRoute(grouped=grouped, capacitance=cap, admm=admm, plan=plan, band=use_band, band_wmin=wmin,
                        polish=pol, loose_eps=eps_loose if loose else 0.0,
                        loose_min_iter=max(int(settings.min_iter), int(settings.min_iter_grouped)) if loose else 0,
                        # sync-free: the group capacitance with the grouped polish only
                        sync_free=bool(sync_free and admm == "gcap" and pol == "grouped"), sparse_cols=sparse_cols)


class _LowRankSolve:
    """One solve_lowrank call: the C structs of its problem and the launches of its route."""

    def __init__(self, qb: QPBatch, lr: LowRank, ws: Workspace, settings: Settings, route: LowRankRoute, tl: _Timeline,
                 groups, eig, sweep, wide_polish: bool, max_rounds: int, sf_rounds):
        self.qb, self.lr, self.ws, self.settings, self.route, self.tl = qb, lr, ws, settings, route, tl
        self.groups, self.eig, self.sweep, self.wide_polish, self.max_rounds, self.sf_rounds = \
            groups, eig, sweep, wide_polish, max_rounds, sf_rounds
        self.lib, self.strm = _lib.load(), _stream()
        self.s, self.sM = settings.to_c(), settings.to_c(sigma=0.0)   # (sM: the capacitances' factor)
        self.SS, self.SSM = ctypes.byref(self.s), ctypes.byref(self.sM)
        # the (lowrank, problem, state) arguments of every launch (a byref keeps its struct alive)
        self.LPS = (ctypes.byref(lr.c_struct()), ctypes.byref(qb.c_struct()), ctypes.byref(ws.c_struct()))
        k_ld = round_up(lr.tmax + qb.mg, 64)
        self.M = ws.lr_buffers(k_ld)        # per-date capacitances M and their inverses
        self.Mcap, self.Minv = ((self.M[k].data_ptr(), k_ld, k_ld * k_ld) for k in ("M", "Minv"))
        self.bd = self.gc = None            # band Gram (_band_setup) and group capacitance
        self.sync_free = route.sync_free    # until the flag read hands over to the host-driven repairs
        self.pg = {}                        # state of the grouped polish pipeline
        self.refactors = self.launches = self.fallbacks = 0

    def group_cap(self):
        """The ADMM's GroupCap, one rho per group: the mean of its dates' initial rho (_rho_floor_q included)."""
        ws, g = self.ws, self.route.plan
        self.gc = ws._gcap = GroupCap(self.qb, ws, g, ws._gcap, mg=self.qb.mg,
                                      gmax=int(g.sizes.max()) if g.ngroups else 0)
        gidx, sizes = g.device_index()
        gr = self.gc.buf["grho"]
        gr.zero_().index_add_(0, gidx, ws.rho)
        gr /= sizes
        torch.index_select(gr, 0, gidx, out=ws.rho)

    def refactor(self, idx, nidx, SS):
        """The capacitance inverses at the current rho: every group's (the kernel agreed a new
        rho per group), or those of problems idx[0..nidx) (None: all)."""
        lib, bd, strm = self.lib, self.bd, self.strm
        if self.gc is not None:
            return self.gc.build(*self.LPS, SS, self.SSM, bd, strm, large=GCAP_FACTOR == "large")
        if self.eig is not None:   # from the per-date eigendecompositions: no factorisation
            return self.eig.form(*self.LPS, SS, self.M["Minv"], idx, nidx, strm)
        if bd is not None:
            _lib.check(lib.pq_lr_capacitance_band(*self.LPS, _ptr(idx), nidx, SS, *bd["cap"], bd["cc"].data_ptr(),
                                                  *self.Mcap, strm), "pq_lr_capacitance_band")
        else:
            _lib.check(lib.pq_lr_capacitance(*self.LPS, _ptr(idx), nidx, SS, *self.Mcap, strm), "pq_lr_capacitance")
        view = _factor_view(self.qb, self.ws, self.M, self.lr.tmax + self.qb.mg, self.ws.rho)
        PM_, SM_ = ctypes.byref(view[0]), ctypes.byref(view[1])
        _lib.check(lib.pq_factor_batched(PM_, SM_, _ptr(idx), nidx, self.SSM, 1, strm), "pq_factor_batched(M)")

    def admm(self, idx, nidx, SS):
        """One launch of the route's ADMM entry point with the settings ``SS``."""
        lib, r, bd, strm, max_iter = self.lib, self.route, self.bd, self.strm, int(self.s.max_iter)
        if r.admm == "gcap":   # group capacitance (admm_gcap.hip)
            nzr, nzv, nzmax = r.sparse_cols if self.qb.mg > 4 else (None, None, 0)
            return lib.pq_admm_lr_gcap(*self.LPS, ctypes.byref(self.gc.c), SS, max_iter, *bd["admm"], _ptr(nzr),
                                       _ptr(nzv), nzmax, strm)
        if r.admm == "sweep":   # two chip-wide launches per iteration (admm_sweep.hip)
            sw = self.sweep
            scr = sw.buffer(self.qb, lib)
            return lib.pq_admm_lr_sweep(*self.LPS, *self.Minv, _ptr(sw.gdates), sw.ngroups, SS, max_iter,
                                        *bd["admm"], int(sw.q_shared), scr.data_ptr(), scr.numel(), strm)
        if r.grouped:   # every group relaunches; solved dates are skipped inside
            g, (nzr, nzv, nzmax) = r.plan, r.sparse_cols
            fused = bd["admm"] if r.admm == "grouped-fused" else (None, 0, 0, None)
            return lib.pq_admm_lr_grouped(*self.LPS, *self.Minv, _ptr(g.gdates), g.ngroups, _ptr(g.urows),
                                          _ptr(g.ucnt), _ptr(g.uoff), g.umax, SS, max_iter, *fused, _ptr(nzr),
                                          _ptr(nzv), nzmax, strm)
        return lib.pq_admm_lr_batched(*self.LPS, *self.Minv, _ptr(idx), nidx, SS, max_iter, strm)

    def admm_rounds(self, idx, nidx, SS, name="admm"):
        """Launch, collect NEED_REFACTOR, refactor, repeat."""
        for _ in range(self.max_rounds):
            _lib.check(self.tl(name, lambda: self.admm(idx, nidx, SS)), "pq_admm_lr")
            self.launches += 1
            if self.sync_free:   # NEED_REFACTOR is caught by the flag at the end
                break
            need = torch.nonzero(self.ws.status == _lib.PQ_NEED_REFACTOR).flatten().to(torch.int32)
            kk = int(need.numel())
            if kk == 0:
                break
            idx, nidx = need.contiguous(), kk
            self.tl("factor", lambda: self.refactor(idx, nidx, SS))
            self.refactors += kk

    def polish_w(self, idx, nidx, SS, name="polish"):
        """The per-date window-form polish of problems idx[0..nidx) (None: all)."""
        lib, qb, ws, tl, strm = self.lib, self.qb, self.ws, self.tl, self.strm
        L_, P_, S_ = self.LPS
        ldk, kmax = ws.ldk, min(qb.ld, 1024)
        final = ldk >= kmax
        bk = self.bd["cap"][:3] if self.bd is not None else (None, 0, 0)
        _lib.check(tl(name, lambda: lib.pq_polish_w_batched(L_, P_, S_, _ptr(idx), nidx, SS, ldk, int(final),
                                                            *bk, strm)), "pq_polish_w_batched")
        if not final:   # free sets larger than the compact scratch: relaunch those with ldk = kmax
            over = torch.nonzero(ws.out[:, _lib.PQ_OUT_ROUNDS] < 0).flatten().to(torch.int32)
            m = int(over.numel())   # host sync: small vector
            if m:
                K2 = torch.empty((m, kmax, kmax), dtype=F64, device=qb.device)
                D2 = torch.empty((m, kmax // 64, 64, 64), dtype=F64, device=qb.device)
                st2 = ws.c_struct(K2, D2)
                over = over.contiguous()
                _lib.check(tl(name, lambda: lib.pq_polish_w_batched(L_, P_, ctypes.byref(st2), _ptr(over), m,
                                                                    SS, kmax, 1, *bk, strm)),
                           "pq_polish_w_batched (relaunch)")

    def pg_start(self, allow_wide: bool):
        """k_pg_init (classification from the ADMM point) + the wide rounds' capacitance."""
        qb, ws = self.qb, self.ws
        rec = ws.pg_record()
        g = self.groups.polish_plan()
        _lib.check(self.lib.pq_polish_grouped_init(*self.LPS, rec.data_ptr(), self.SS, self.strm),
                   "pq_polish_grouped_init")
        if ws._pg_pass is None or ws._pg_pass.numel() < g.ngroups * _lib.PQ_PG_PASS_SCRATCH:
            ws._pg_pass = torch.empty(g.ngroups * _lib.PQ_PG_PASS_SCRATCH, dtype=F64, device=qb.device)
        # free sets beyond the LDS solve (k_pg_init left each date's free count in PQ_PG_K): the
        # wide rounds' group capacitance, built once for the whole polish
        wide = None
        if allow_wide and self.wide_polish and bool((rec[:, _lib.PQ_PG_K] > min(ws.ldk, 128)).any()):   # host sync
            wide = _pg_wide_setup(qb, self.lr, ws, g, self.bd, rec, self.settings, self.route.sparse_cols, self.strm)
        # (the state a replayed sync-free stage hands back: rounds run, the record, a round's arguments)
        self.pg = dict(rounds=0, rec=rec, keep=(g, wide), round=(
            *self.LPS, rec.data_ptr(), ws.ldk, _ptr(g.gdates), g.ngroups, _ptr(g.urows), _ptr(g.ucnt), _ptr(g.uoff),
            g.umax, self.SS, ws._pg_pass.data_ptr(), ctypes.byref(wide) if wide is not None else None, self.strm))

    def pg_round(self):
        _lib.check(self.lib.pq_polish_grouped_round(*self.pg["round"]), "pq_polish_grouped_round")
        self.pg["rounds"] += 1

    def pg_rounds_host(self):
        """The remaining rounds, each followed by a host check for dates still pending."""
        rec = self.pg["rec"]
        while self.pg["rounds"] < int(self.s.polish_rounds):
            if self.pg["rounds"] >= 2 and not bool((rec[:, _lib.PQ_PG_STATE] == _lib.PQ_PG_PENDING).any()):   # sync
                break
            self.pg_round()

    def polish_grouped(self):
        """Grouped polish pipeline (polish_g.hip) for every date; the dates it hands back take the per-date one."""
        self.pg_start(True)
        self.pg_round()
        self.pg_rounds_host()
        self.pg_finish()

    def polish_sync_free(self):
        """The grouped polish with a fixed number of rounds and no host check (dates done early skip the later
        rounds' kernels), then one device flag in ws._sf_flag: anything left for the host-driven repairs (dates
        pending, handed back or rejected, or an ADMM refactor).  Returns the pipeline state (a copy)."""
        ws, rounds = self.ws, int(self.s.polish_rounds)
        self.pg_start(False)
        for _ in range(min(int(self.sf_rounds or rounds), rounds)):
            self.pg_round()
        if ws._sf_flag is None:
            ws._sf_flag = torch.zeros((), dtype=torch.bool, device=ws.device)
        rec = self.pg["rec"]
        if self.pg["rounds"] > 0 and not SF_FLAG_HOST:
            # the last round's k_pg_post noted the dates left for the host (pg_record.h, R_SFLAG): one launch
            left = rec[0, _lib.PQ_PG_SFLAG:_lib.PQ_PG_SFLAG + 1].view(torch.int64)[0]
            torch.ne(left, 0, out=ws._sf_flag)
        else:   # no round ran: nothing has counted
            ws._sf_flag.copy_(sf_flag_torch(rec, ws.status))
        return dict(self.pg)

    def pg_finish(self):
        """The dates the pipeline handed back: the per-date polish from their ADMM point."""
        ws = self.ws
        fb = torch.nonzero(self.pg["rec"][:, _lib.PQ_PG_STATE] == _lib.PQ_PG_FALLBACK).flatten().to(torch.int32)
        m = self.fallbacks = int(fb.numel())
        if m:
            ws.pg_fallback = fb   # (diagnostics)
            if self.route.loose_eps > 0:   # stopped at the loose eps: resume those to eps first
                ws.status[fb.long()] = _lib.PQ_UNSOLVED
                self.admm_rounds(fb.contiguous(), m, self.SS, name="admm (resume, inside polish)")
            # two refinement steps per round for the hand-offs (vertex cycling, failed
            # factorisations): config 5's fallback polish 31.3 -> 7.5 ms
            # (profiles/r02k_bench_config5_qrel30.log -> r02l_bench_config5_fallback_refine2.log)
            sfb = self.settings.to_c(refine_iters=max(self.settings.refine_iters, 2))
            self.polish_w(fb.contiguous(), m, ctypes.byref(sfb), name="polish (fallback, inside polish)")

    def result(self) -> BatchResult:
        return _batch_result(self.qb, self.ws, refactors=self.refactors, admm_launches=self.launches,
                             polish_fallbacks=self.fallbacks, capacitance=self.route.capacitance)


def solve_lowrank(qb: QPBatch, lr: LowRank, settings: Settings | None = None,
                  ws: Workspace | None = None, max_rounds: int = 64, events: list | None = None,
                  polish: bool = True, groups: "GroupPlan | None" = None, band: bool = True,
                  fuse: bool = True, grouped_polish: bool = True, gcap: bool = True,
                  eig: "EigCap | None" = None, wide_polish: bool = True, sync_free: bool = False,
                  graphs: "StageGraphs | None" = None, sf_rounds: int | None = None,
                  host_work=None, sweep: "SweepPlan | None" = None) -> BatchResult:
    """Woodbury-form solve for T + mg < n: K2 = capacitance SYRK + Cholesky/inverse of the
    k x k matrices M, K3 = low-rank ADMM over the shared window rows (grouped over sliding
    windows when a GroupPlan is given), K4 = window-form polish.  qb.P is never read (it
    may be None): P is the window (lr) throughout.  Which kernels run is decided once, by
    lowrank_route.

    ``sync_free`` (group capacitance with the grouped polish, no wide rounds): the stages
    run without any host synchronisation -- one ADMM launch, ``sf_rounds`` polish rounds
    (default settings.polish_rounds) -- and one flag read at the end decides whether the
    usual host-driven repairs must run (an adaptive-rho refactorisation: the whole solve is
    redone the host-driven way; dates still pending, handed back, or rejected: the remaining
    rounds, the per-date polish and the ADMM retry, exactly as without it).  With ``graphs``
    (StageGraphs) the sync-free stages are captured once and replayed.  ``host_work`` (a
    callable, sync-free only): the caller's host work that needs no result, run while the
    device works, just before the flag read.  ``sweep`` (SweepPlan: groups of up to 64
    problems sharing one window, porqua_amd.sweep): the fused ADMM runs as pq_admm_lr_sweep
    (two chip-wide launches per iteration) instead of one workgroup per group."""
    settings = settings or Settings()
    ws = ws or Workspace(qb, dense=False)
    if not lowrank_applicable(qb, lr):
        raise _lib.PorquaHipError(f"low-rank form not applicable (k={lr.tmax + qb.mg}, n={qb.n})")
    route = lowrank_route(qb, lr, ws, groups, settings, polish=polish, band=band, fuse=fuse,
                          grouped_polish=grouped_polish, gcap=gcap, wide_polish=wide_polish, sync_free=sync_free,
                          eig=eig, sweep=sweep)
    tl = _Timeline(events, graphs if route.sync_free else None)
    if tl.graphs is not None:
        tl.graphs.begin()
    c = _LowRankSolve(qb, lr, ws, settings, route, tl, groups, eig, sweep, wide_polish, max_rounds, sf_rounds)
    # what bench.py and the tests read: the plan and the kernel the ADMM runs on
    ws.gcap_groups = route.plan if route.admm == "gcap" else None
    ws.sweep_admm = sweep if route.admm == "sweep" else None
    ws.pg_fallback = None
    s_init = _init_settings(settings)
    _lib.check(c.lib.pq_init_state_lr(*c.LPS, None, 0, ctypes.byref(s_init), c.strm), "pq_init_state_lr")
    _rho_floor_q(qb, ws, settings, in_kernel=s_init.rho0_qrel > 0)
    if band:
        c.bd = tl("gram", lambda: _band_setup(qb, lr, c.strm, w_min=route.band_wmin))
    ws.band_shape = (c.bd["nrows"], c.bd["W"]) if c.bd is not None else None   # (the bench's gram rate)
    if route.admm == "gcap":
        c.group_cap()
    tl("factor", lambda: c.refactor(None, 0, c.SS))

    SS_admm = c.SS
    if route.loose_eps > 0:   # the ADMM only has to predict the active set for the grouped polish
        sl = settings.to_c(eps_abs=route.loose_eps, eps_rel=route.loose_eps, min_iter=route.loose_min_iter)
        SS_admm = ctypes.byref(sl)
    c.admm_rounds(None, 0, SS_admm)

    if c.sync_free:
        c.pg = dict(tl("polish", c.polish_sync_free))   # (a replayed graph does not run the function)
        if host_work is not None:
            host_work()
        if not bool(ws._sf_flag.item()):   # the one host sync of the step: nothing left to repair
            return c.result()
        if bool((ws.status == _lib.PQ_NEED_REFACTOR).any() | (ws.status == _lib.PQ_UNSOLVED).any()):
            # an adaptive-rho refactorisation was requested: redo the whole solve host-driven.
            # Not forwarded: sync_free, graphs and sf_rounds (the redo is the host-driven solve),
            # host_work (it ran above) and sweep (the redo takes the group capacitance again,
            # which has no sweep form)
            return solve_lowrank(qb, lr, settings=settings, ws=ws, max_rounds=max_rounds, events=events,
                                 polish=polish, groups=groups, band=band, fuse=fuse, grouped_polish=grouped_polish,
                                 gcap=gcap, eig=eig, wide_polish=wide_polish)
        tl.graphs = None       # the repairs below are host-driven
        c.sync_free = False    # (admm_rounds checks for refactorisations again)
        c.pg_rounds_host()     # dates still pending: the remaining rounds
        c.pg_finish()          # dates handed back: the per-date polish
    elif route.polish == "grouped":
        tl("polish", c.polish_grouped)
    elif route.polish == "per-date":
        c.polish_w(None, 0, c.SS)
    if route.polish != "none":
        # one host sync: nothing rejected (the usual case) skips both repairs
        rejected = bool((ws.status == _lib.PQ_SOLVED_INACCURATE).any().item())
        rp = _repolish_set(ws, settings) if rejected else None
        if rp is not None:      # polish rejected: polish again with more refinement steps
            pidx, pn, s3 = rp
            c.polish_w(pidx, pn, ctypes.byref(s3))
        retry = _retry_set(ws, settings) if rejected else None
        if retry is not None:   # polish rejected: resume ADMM to eps_retry, polish again
            ridx, rn, s2 = retry
            c.admm_rounds(ridx, rn, ctypes.byref(s2))
            s4 = settings.to_c(refine_iters=max(settings.refine_iters, settings.refine_retry))
            c.polish_w(ridx, rn, ctypes.byref(s4))
    return c.result()


def factor_only(qb: QPBatch, invert: bool = False, sigma: float = 0.0):
    """Batched Cholesky of P_eff (mg = 0, no box): returns (Workspace, info) -- the isPD
    test of src/helper_functions.py:61-67 on the device."""
    lib = _lib.load()
    s = Settings(sigma=sigma).to_c()
    ws = Workspace(qb)
    pb = qb.c_struct()
    pb.mg = 0
    pb.lb = pb.ub = None
    st = ws.c_struct()
    strm = _stream()
    _lib.check(lib.pq_init_state(ctypes.byref(pb), ctypes.byref(st), None, 0, ctypes.byref(s), strm), "init")
    _lib.check(lib.pq_factor_batched(ctypes.byref(pb), ctypes.byref(st), None, 0, ctypes.byref(s),
                                     2 if invert else 0, strm), "pq_factor_batched")
    return ws, ws.info


# ----------------------------------------------------------------------------------------
# Windows and K1
# ----------------------------------------------------------------------------------------


def window_rows(dates: np.ndarray, rebdates, width: int):
    """Per-date row lists of ``data[data.index <= rebdate].tail(width)`` minus weekends
    (src/builders.py:208-211).  Returns (rows int32 [B, Tmax], tlen int32 [B])."""
    dates = np.asarray(dates, dtype="datetime64[D]")
    reb = np.asarray(rebdates, dtype="datetime64[D]")
    ends = np.searchsorted(dates, reb, side="right")
    starts = np.maximum(0, ends - int(width))
    B = len(ends)
    weekday = (dates.astype("int64") + 3) % 7 < 5
    # the weekdays of [s, e) are the positions wpos[cw[s] .. cw[e]) (prefix counts)
    wpos = np.flatnonzero(weekday).astype(np.int32)
    cw = np.concatenate([[0], np.cumsum(weekday)]).astype(np.int64)
    first = cw[starts]
    tlen = (cw[ends] - first).astype(np.int32)
    tmax = max(1, int(tlen.max())) if B else 1
    if not len(wpos):
        return np.zeros((B, tmax), dtype=np.int32), tlen
    # int32 index arithmetic; a calendar without weekend rows (the usual return panel) needs
    # no position lookup at all (wpos is the identity)
    j = np.arange(tmax, dtype=np.int32)[None, :]
    idx = first.astype(np.int32)[:, None] + j
    if len(wpos) != len(dates):
        idx = wpos[np.minimum(idx, len(wpos) - 1)]
    if B and int(tlen.min()) == tmax:   # every window full (the usual backtest): nothing to mask
        return idx.astype(np.int32, copy=False), tlen
    rows = idx * (j < tlen[:, None])
    return rows.astype(np.int32, copy=False), tlen


def slide_plan(rows, tlen, group: int = 32, smax: int = 64, smin: int = 1):
    """Host plan for pq_cov_slide_batched: ``(gstart int32 [G+1], shift int32 [B])``.

    Date d joins the group of date d-1 when its window is that window shifted by
    smin <= s <= smax rows (same length, rows[d][:T-s] == rows[d-1][s:T]) and the group
    holds fewer than ``group`` dates; otherwise d starts a new group (a full-SYRK anchor).
    smin = 0 also joins identical windows (several problems of one date, e.g. a
    risk-aversion sweep) -- the grouped ADMM accepts that, the sliding K1 does not."""
    rows = np.asarray(rows)
    tlen = np.asarray(tlen)
    B, tmax = rows.shape
    shift = np.zeros(B, dtype=np.int32)
    if B > 1:
        col = np.arange(tmax)
        prev, cur = rows[:-1], rows[1:]
        tp, tc = tlen[:-1], tlen[1:]
        # s = #rows of the previous window before the current window's first row; only
        # s <= smax can join, so the first smax + 1 columns decide it
        h = min(tmax, int(smax) + 1)
        # windows that are one contiguous run of panel rows (no gap: last - first = T - 1)
        # of the same length, the current one starting exactly s rows after the previous one,
        # are that window shifted by s -- no element compare needed.  (Without the start check
        # a later window starting EARLIER -- descending or shuffled dates -- counts s = 0 and
        # would pass as identical.)
        last = rows[np.arange(B), np.maximum(tlen - 1, 0)]
        contig = (last - rows[:, 0]) == (tlen - 1)
        if contig.all():   # (the same count from the window starts alone)
            s = np.minimum(np.clip(cur[:, 0].astype(np.int64) - prev[:, 0], 0, tp), h)
        else:
            s = ((prev[:, :h] < cur[:, :1]) & (col[None, :h] < tp[:, None])).sum(1)
        cand = (tp == tc) & (tc > 1) & (s >= smin) & (s <= smax)
        match = cand & contig[:-1] & contig[1:] & ((cur[:, 0] - prev[:, 0]) == s)
        need = cand & ~match
        for sv in np.unique(s[need]).tolist():   # rows[d][:T-s] == rows[d-1][s:T], per shift value
            sel = np.flatnonzero(need & (s == sv))
            w = tmax - sv
            ok = ((prev[sel, sv:] == cur[sel, :w]) | (col[None, :w] >= (tc[sel] - sv)[:, None])).all(1)
            match[sel[ok]] = True
        good = cand & match
        shift[1:] = np.where(good, s, 0)
    else:
        good = np.zeros(0, dtype=bool)
    joins = np.concatenate([[False], good])
    # runs of joined dates, cut every ``group`` dates: d starts a group when it does not
    # join its predecessor or sits at a multiple of ``group`` inside its run
    run_start = np.maximum.accumulate(np.where(~joins, np.arange(B), 0)) if B else np.zeros(0, np.int64)
    starts = np.flatnonzero((np.arange(B) - run_start) % max(int(group), 1) == 0)
    return np.concatenate([starts, [B]]).astype(np.int32), shift


class SlidePlan:
    """Device copy of a slide_plan (see pq_cov_slide_batched)."""

    def __init__(self, rows, tlen, device, group: int = 32, smax: int = 64):
        gs, sh = slide_plan(rows, tlen, group, smax)
        self.ngroups = len(gs) - 1
        self.gstart = torch.from_numpy(gs).to(device)
        self.shift = torch.from_numpy(sh).to(device)


GROUP_MAX_DATES = 16     # MFMA N of the grouped ADMM (admm_grp.hip GMAX)
# dates per group of the group-capacitance ADMM with its two MFMA column blocks (admm_gcap.hip,
# NB = 2: one 512-thread workgroup per CU); PQ_GCAP_GMAX=16 keeps the 16-date groups (A/B)
GCAP_MAX_DATES = int(os.environ.get("PQ_GCAP_GMAX", "32"))
# the 32-date groups also for the wide form (column-sparse general rows, config 4's sector
# caps); PQ_GCAP32_WIDE=0: 16-date groups there (A/B)
GCAP32_WIDE = os.environ.get("PQ_GCAP32_WIDE", "1") != "0"
GCAP_FACTOR = os.environ.get("PQ_GCAP_FACTOR", "batched")   # (A/B) "large": K2L for the group factor
GROUP_MAX_UNION = 320    # union rows per group (admm_grp.hip UMAXG)


# (A/B) PQ_RHO_FLOOR_HOST=1: the |q| floor of the initial rho by torch after the init kernel (_rho_floor_q)
# instead of inside it; PQ_SF_FLAG_HOST=1: the sync-free flag by the torch expression (sf_flag_torch)
# instead of from the polish's own count
RHO_FLOOR_HOST = os.environ.get("PQ_RHO_FLOOR_HOST", "0") != "0"
SF_FLAG_HOST = os.environ.get("PQ_SF_FLAG_HOST", "0") != "0"
SWEEP_ADMM = os.environ.get("PQ_SWEEP_ADMM", "1") != "0"   # (A/B) 0: the sweep's groups on k_admm_grp


class SweepPlan:
    """Problem groups for pq_admm_lr_sweep (admm_sweep.hip): runs of up to 64 consecutive
    problems that share one window and its centring (the risk-aversion row of a rebalance
    date, porqua_amd.sweep), with the kernel's scratch (per-problem records, per-chunk
    partials, the pass-2 operand).  ``q_shared``: the problems of a group share q as well.

    Precondition of the kernel (not checked on the device): gdates[g + 1] - gdates[g] <= 64
    for every group -- a group's problems are the 64 MFMA columns of one workgroup.  The plan
    built here never emits a larger group (``counts`` above 64 are cut into runs of 64 and a
    remainder); a hand-made gdates must keep to it."""

    GMAX = 64

    def __init__(self, counts, device, q_shared: bool = False):
        self.q_shared = bool(q_shared)
        starts, b = [], 0
        for c in counts:
            starts.extend(range(b, b + int(c), self.GMAX))
            b += int(c)
        starts.append(b)
        self.gdates = torch.tensor(starts, dtype=torch.int32, device=device)
        self.ngroups = len(starts) - 1
        self.scratch = None

    def applicable(self, qb: "QPBatch", lr: "LowRank", k_ld: int) -> bool:
        return (SWEEP_ADMM and self.ngroups > 0 and lr.tmax <= 256 and k_ld <= 256 and qb.mg <= 4
                and qb.lb is not None and qb.ub is not None and qb.shared)

    def buffer(self, qb: "QPBatch", lib) -> torch.Tensor:
        need = int(lib.pq_sweep_scratch_doubles(qb.n, qb.batch, self.ngroups))
        if self.scratch is None or self.scratch.numel() < need:
            self.scratch = torch.empty(need, dtype=F64, device=qb.device)
        return self.scratch


class GroupPlan:
    """Date groups for pq_admm_lr_grouped: runs of consecutive dates whose windows slide
    (slide_plan), at most ``gmax`` dates and ``umax`` union rows each.  ``ok`` is False
    when some window cannot be grouped (the per-date kernel is used then)."""

    def __init__(self, rows, tlen, device, gmax: int = GROUP_MAX_DATES, umax: int = GROUP_MAX_UNION,
                 smax: int = 64, cus: int = 256, gmin: int = 4, breaks=None, polish_full: bool = False):
        """``breaks`` (bool per problem, optional): True starts a new group at that problem
        (e.g. the risk-aversion buckets of porqua_amd.sweep, whose problems may share a
        capacitance only within a rho bucket).  ``polish_full``: polish_plan() builds a second plan
        of full 16-date groups for the grouped polish (a second host pass over the windows: worth
        it for a batch solved repeatedly, e.g. the bench workloads)."""
        rows = np.asarray(rows)
        tlen = np.asarray(tlen)
        B = len(tlen)
        self._host = (rows, tlen, device, umax, smax, breaks, cus, gmax)
        self._polish_full = polish_full
        self._polish_plan = None
        self._gcap_plan = None
        self._gmin = gmin
        # balance: one group per CU per round (one 512-thread workgroup fits a CU), as few
        # rounds as gmax allows, groups as even as possible within them
        rounds = max(1, -(-B // (gmax * cus)))
        gmax = max(1, min(gmax, max(gmin, -(-B // (rounds * cus)))))
        self.ok = B > 0 and int(tlen.min()) >= 2 and int(tlen.max()) <= umax
        gs, sh = slide_plan(rows, tlen, group=gmax, smax=smax, smin=0)
        # windows that are runs of consecutive panel rows, each joined one starting exactly its
        # shift after its predecessor: every union is then a run too (the fast path below; a
        # shift of a whole window or more joins disjoint windows, whose union has gaps)
        contig_all = bool(B) and bool(((rows[np.arange(B), np.maximum(tlen - 1, 0)] - rows[:, 0]) == (tlen - 1)).all()
                                      and ((sh[1:] == 0) | (rows[1:, 0] - rows[:-1, 0] == sh[1:])).all())
        groups = []
        # a slide group whose whole union fits (first window + every later shift <= umax) is
        # one date group; only the others are cut greedily, date by date
        cs = np.concatenate([[0], np.cumsum(sh[1:], dtype=np.int64)]) if B else np.zeros(1, np.int64)
        fits = (tlen[gs[:-1]] + cs[gs[1:] - 1] - cs[gs[:-1]]) <= umax if B else np.zeros(0, bool)
        tl_l, sh_l = tlen.tolist(), sh.tolist()
        for a, b, f in zip(gs[:-1].tolist(), gs[1:].tolist(), fits.tolist()):
            if f:
                groups.append((a, b))
                continue
            start, U = a, tl_l[a]
            for d in range(a + 1, b):
                if U + sh_l[d] > umax:
                    groups.append((start, d))
                    start, U = d, tl_l[d]
                else:
                    U += sh_l[d]
            groups.append((start, b))
        if breaks is not None:
            brk = np.flatnonzero(np.asarray(breaks, dtype=bool))
            split = []
            for a, b in groups:
                cut = [a] + [int(c) for c in brk if a < c < b] + [b]
                split += list(zip(cut[:-1], cut[1:]))
            groups = split
        self.ngroups = len(groups)
        self.umax = umax
        gdates = np.array([a for a, _ in groups] + [B], dtype=np.int32)
        urows = np.zeros((max(1, self.ngroups), umax), dtype=np.int32)
        ucnt = np.zeros(max(1, self.ngroups), dtype=np.int32)
        uoff = np.zeros(B, dtype=np.int32)
        if B and self.ngroups:
            # a group's union = its first window, then the rows each later date adds (its last
            # sh[d] window rows); every (date, column) entry gathered at once
            sizes = np.diff(gdates)
            gof = np.repeat(np.arange(self.ngroups), sizes)                 # group of each date
            isfirst = np.zeros(B, dtype=bool)
            isfirst[gdates[:-1]] = True
            shd = np.where(isfirst, 0, sh).astype(np.int64)
            cnt = np.where(isfirst, tlen, shd).astype(np.int64)             # entries per date
            col0 = np.where(isfirst, 0, tlen - shd)
            cum = np.cumsum(shd)
            uoff[:] = cum - cum[gdates[:-1]][gof]                           # sum of shifts since the group start
            cnts = np.add.reduceat(cnt, gdates[:-1]) if self.ngroups else np.zeros(0, np.int64)
            over = cnts > umax
            if over.any():
                self.ok = False
            g0 = gdates[:-1]
            if contig_all:
                # every window one run of consecutive panel rows (daily / monthly calendars
                # without gaps): a group's union is the run from its first window's first row
                u = np.arange(umax)[None, :]
                urows[:] = np.where((u < cnts[:, None]) & ~over[:, None], rows[g0, 0][:, None] + u, 0)
            else:
                estart = np.concatenate([[0], np.cumsum(cnt)])
                tot = int(estart[-1])
                dte = np.repeat(np.arange(B), cnt)
                k = np.arange(tot) - estart[dte]
                vals = rows[dte, col0[dte] + k]
                gstart_e = estart[g0]                                       # first entry of each group
                pos = np.arange(tot) - gstart_e[gof[dte]]
                keep = ~over[gof[dte]]
                urows[gof[dte][keep], pos[keep]] = vals[keep]
            ucnt[:] = np.where(over, 0, cnts)
        self.sizes = np.diff(gdates)
        gidx = np.repeat(np.arange(max(self.ngroups, 0), dtype=np.int32), self.sizes) if B else np.zeros(0, np.int32)
        # widest union span in panel rows (the band Gram must cover it for the group capacitance)
        if self.ngroups and ucnt.max() > 0:
            valid = np.arange(umax)[None, :] < ucnt[:, None]
            hi = np.where(valid, urows, np.iinfo(np.int32).min).max(1)
            lo = np.where(valid, urows, np.iinfo(np.int32).max).min(1)
            self.span_max = int((hi - lo + 1)[ucnt > 0].max())
        else:
            self.span_max = 0
        self.ucnt_max = int(ucnt.max()) if self.ngroups else 0
        # rank of the Woodbury correction of a date: union rows outside its window + the mean
        self.corr_max = int((ucnt[gidx] - tlen).max()) + 1 if B else 1
        self.gdates = torch.from_numpy(gdates).to(device)
        self.urows = torch.from_numpy(urows).to(device)
        self.ucnt = torch.from_numpy(ucnt).to(device)
        self.uoff = torch.from_numpy(uoff).to(device)
        self.gidx = torch.from_numpy(gidx).to(device)
        self._dev_index = None

    def polish_plan(self) -> "GroupPlan":
        """The plan of the grouped polish: full 16-date groups (its window passes run split
        over 4 workgroups per group, so fewer, fuller groups read fewer union rows; measured at
        the config-3 shape, profiles/r03i_bench_gmin*.log: polish 5.26 -> 4.92 ms at 16 dates per
        group, while the ADMM wants the CU-balanced size: 8.06 -> 8.51 ms)."""
        if not self._polish_full:
            return self
        if self._polish_plan is None:
            rows, tlen, device, umax, smax, breaks, cus, gmax0 = self._host
            full = self.ngroups == 0 or int(self.sizes.max()) >= min(gmax0, GROUP_MAX_DATES)
            # same breaks (e.g. rho buckets) and CU count: polish groups never straddle a break
            self._polish_plan = None if full else GroupPlan(rows, tlen, device, umax=umax, smax=smax, cus=cus,
                                                            gmax=gmax0, gmin=gmax0, breaks=breaks)
            if full:
                self._polish_full = False
        return self._polish_plan if self._polish_plan is not None else self

    def gcap_plan(self) -> "GroupPlan":
        """The plan of the group-capacitance ADMM (admm_gcap.hip) for register-resident general
        rows (mg <= 4): CU-balanced groups of up to GCAP_MAX_DATES dates (its 32-date form: one
        workgroup per CU streams one union for all of them -- half the union traffic and half the
        group factorisations of two 16-date groups; config 3: 475 groups of 10 -> 250 of 19).
        This plan itself when that changes nothing (small batches, GCAP_MAX_DATES <= 16)."""
        if self._gcap_plan is None:
            rows, tlen, device, umax, smax, breaks, cus, gmax0 = self._host
            g = self
            if GCAP_MAX_DATES > gmax0 and self.ngroups > 0:
                g32 = GroupPlan(rows, tlen, device, gmax=min(GCAP_MAX_DATES, 32), umax=umax, smax=smax, cus=cus,
                                gmin=self._gmin, breaks=breaks)
                if g32.ok and g32.ngroups < self.ngroups and int(g32.sizes.max()) > gmax0:
                    g = g32
            self._gcap_plan = g
        return self._gcap_plan

    def device_index(self):
        """(group of each date as int64, dates per group as FP64) on the device, built once."""
        if self._dev_index is None:
            self._dev_index = (self.gidx.long(), torch.from_numpy(self.sizes.astype(np.float64)).to(self.gidx.device))
        return self._dev_index


class Panel:
    """A device-resident return panel (D_total x n, row-major) with optional benchmark."""

    def __init__(self, returns, bm=None, device=None):
        self.device = device or default_device()
        R = returns if isinstance(returns, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(returns, dtype=np.float64))
        self.R = R.to(self.device, dtype=F64).contiguous()
        self.D, self.n = self.R.shape
        self.bm = None
        self._has_nan = None
        if bm is not None:
            y = bm if isinstance(bm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(bm, dtype=np.float64).reshape(-1))
            self.bm = y.to(self.device, dtype=F64).contiguous()

    def window_sumsq(self, rows, tlen, mu=None, out=None):
        """diag(Xc'Xc) of every window (mu None: diag X'X) -> (B, round_up(n, 64))."""
        lib = _lib.load()
        B, tmax = rows.shape
        if out is None:
            out = torch.zeros((B, round_up(self.n, 64)), dtype=F64, device=self.device)
        _lib.check(lib.pq_window_sumsq(_ptr(self.R), self.R.stride(0), self.n, _ptr(rows), _ptr(tlen), tmax, B,
                                       _ptr(mu), 0 if mu is None else mu.stride(0), _ptr(out), out.stride(0),
                                       _stream()), "pq_window_sumsq")
        return out

    def window_moments_grouped(self, groups: "GroupPlan", tlen, mu, dg):
        """Window means and diag(Xc'Xc) of every date of a GroupPlan in one sliding pass over
        each group's union rows (pq_window_moments_grouped), into ``mu`` and ``dg``."""
        lib = _lib.load()
        _lib.check(lib.pq_window_moments_grouped(_ptr(self.R), self.R.stride(0), self.n, _ptr(groups.gdates),
                                                 groups.ngroups, _ptr(groups.urows), groups.umax,
                                                 _ptr(groups.uoff), _ptr(tlen), _ptr(mu), mu.stride(0), _ptr(dg),
                                                 dg.stride(0), _stream()), "pq_window_moments_grouped")
        return mu, dg

    def window_geomeans_grouped(self, groups: "GroupPlan", tlen, out=None):
        """Geometric window means (MeanEstimator.estimate_geometric) of every date of a
        GroupPlan in one sliding pass per group (pq_window_geomean_grouped) -> (B, round_up(n, 64))."""
        lib = _lib.load()
        B = int(tlen.shape[0])
        mu = out if out is not None else torch.zeros((B, round_up(self.n, 64)), dtype=F64, device=self.device)
        _lib.check(lib.pq_window_geomean_grouped(_ptr(self.R), self.R.stride(0), self.n, _ptr(groups.gdates),
                                                 groups.ngroups, _ptr(groups.urows), groups.umax,
                                                 _ptr(groups.uoff), _ptr(tlen), _ptr(mu), mu.stride(0),
                                                 _stream()), "pq_window_geomean_grouped")
        return mu

    def rows_to_device(self, rows, tlen):
        r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)
        t = torch.from_numpy(np.ascontiguousarray(tlen, dtype=np.int32)).to(self.device)
        return r, t

    def window_means(self, rows, tlen, geometric=False, out=None):
        lib = _lib.load()
        B, tmax = rows.shape
        mu = out if out is not None else torch.zeros((B, round_up(self.n, 64)), dtype=F64, device=self.device)
        fn = lib.pq_window_geomean if geometric else lib.pq_window_mean
        _lib.check(fn(_ptr(self.R), self.R.stride(0), self.n, _ptr(rows), _ptr(tlen), tmax, B, _ptr(mu),
                      mu.stride(0), _stream()), "window means")
        return mu

    def window_nanmeans(self, rows, tlen, geometric=False, out=None):
        """Column means over the present rows of every window (NaN-aware; pandas skipna),
        arithmetic or geometric -> (B, round_up(n, 64))."""
        lib = _lib.load()
        B, tmax = rows.shape
        mu = out if out is not None else torch.zeros((B, round_up(self.n, 64)), dtype=F64, device=self.device)
        _lib.check(lib.pq_window_nanmean(_ptr(self.R), self.R.stride(0), self.n, _ptr(rows), _ptr(tlen), tmax, B,
                                         _ptr(mu), mu.stride(0), int(geometric), _stream()), "pq_window_nanmean")
        return mu

    @property
    def has_nan(self) -> bool:
        if self._has_nan is None:
            self._has_nan = bool(torch.isnan(self.R).any().item())
        return self._has_nan

    def cov_pairwise(self, rows, tlen, out=None):
        """Pairwise-complete covariance of windows with missing values (pandas
        DataFrame.cov() with NaN, src/covariance.py:65-66) -> (B, ld, ld); NaN where a pair
        has fewer than 2 common rows."""
        lib = _lib.load()
        B, tmax = rows.shape
        ld = round_up(self.n, 64)
        c = torch.nan_to_num(self.window_nanmeans(rows, tlen), nan=0.0)   # all-missing column: no shift
        if out is None:
            out = torch.empty((B, ld, ld), dtype=F64, device=self.device)
        _lib.check(lib.pq_cov_pairwise_batched(_ptr(self.R), self.R.stride(0), self.n, _ptr(rows), _ptr(tlen), tmax,
                                               B, _ptr(c), c.stride(0), _ptr(out), ld, out.stride(0), _stream()),
                   "pq_cov_pairwise_batched")
        return out

    def cov(self, rows, tlen, mode=0, out=None, mu=None, plan: SlidePlan | None = None,
            lower_only: bool = False):
        """K1: per-date centred covariance (mode 0, ddof=1) or Gram X'X (mode 1) -> (B, ld, ld).
        With a SlidePlan, overlapping windows are built by rank-2s updates (same result);
        ``lower_only`` (SlidePlan only) leaves the strictly-upper off-diagonal tiles unwritten."""
        lib = _lib.load()
        B, tmax = rows.shape
        ld = round_up(self.n, 64)
        if mode == 0 and mu is None:
            mu = self.window_means(rows, tlen)
        if out is None:
            out = torch.empty((B, ld, ld), dtype=F64, device=self.device)
        mp = _ptr(mu) if mode == 0 else None
        ms = mu.stride(0) if mode == 0 else 0
        if plan is not None:
            _lib.check(lib.pq_cov_slide_batched(_ptr(self.R), self.R.stride(0), self.n, _ptr(rows), _ptr(tlen),
                                                tmax, B, mode, mp, ms, _ptr(out), ld, out.stride(0),
                                                _ptr(plan.gstart), plan.ngroups, _ptr(plan.shift),
                                                1 if lower_only else 0, _stream()),
                       "pq_cov_slide_batched")
            return out
        _lib.check(lib.pq_cov_batched(_ptr(self.R), self.R.stride(0), self.n, _ptr(rows), _ptr(tlen), tmax, B,
                                      mode, mp, ms, _ptr(out), ld, out.stride(0), _stream()), "pq_cov_batched")
        return out

    def gram_xy(self, rows, tlen):
        lib = _lib.load()
        if self.bm is None:
            raise ValueError("Benchmark return series data is missing.")
        B, tmax = rows.shape
        ld = round_up(self.n, 64)
        xty = torch.zeros((B, ld), dtype=F64, device=self.device)
        yty = torch.zeros(B, dtype=F64, device=self.device)
        _lib.check(lib.pq_gram_xy_batched(_ptr(self.R), self.R.stride(0), self.n, _ptr(self.bm), _ptr(rows),
                                          _ptr(tlen), tmax, B, _ptr(xty), xty.stride(0), _ptr(yty),
                                          _stream()), "pq_gram_xy_batched")
        return xty, yty

    def gram_xy_grouped(self, groups: "GroupPlan", tlen, dg=None, xty=None):
        """gram_xy for the dates of a GroupPlan in one sliding pass per group
        (pq_gram_xy_grouped: O(n) per date after each group's first window); ``dg`` (optional,
        (B, >= n)) receives diag(X'X) of every window from the same pass."""
        lib = _lib.load()
        if self.bm is None:
            raise ValueError("Benchmark return series data is missing.")
        B = int(tlen.shape[0])
        ld = round_up(self.n, 64)
        if xty is None:
            xty = torch.zeros((B, ld), dtype=F64, device=self.device)
        yty = torch.zeros(B, dtype=F64, device=self.device)
        _lib.check(lib.pq_gram_xy_grouped(_ptr(self.R), self.R.stride(0), self.n, _ptr(self.bm), _ptr(groups.gdates),
                                          groups.ngroups, _ptr(groups.urows), groups.umax, _ptr(groups.uoff),
                                          _ptr(tlen), _ptr(xty), xty.stride(0), _ptr(yty), _ptr(dg),
                                          0 if dg is None else dg.stride(0), _stream()), "pq_gram_xy_grouped")
        return xty, yty



class PeriodPlan:
    """Device tables of one simulation launch: first panel row and row count of every
    holding period, the offset of its returns in the flattened series and (for the fixed
    cost) the calendar day of every return.  Built once, reusable across launches."""

    def __init__(self, row0, nrows, ret_day=None, device=None, panel_rows=None):
        row0 = np.asarray(row0, dtype=np.int64)
        nrows = np.asarray(nrows, dtype=np.int64)
        if len(row0) != len(nrows):
            raise ValueError("PeriodPlan: one (row0, nrows) per period")
        if len(row0) and (row0.min() < 0 or nrows.min() < 1 or
                          (panel_rows is not None and (row0 + nrows).max() > panel_rows)):
            raise ValueError("PeriodPlan: period rows outside the panel")
        self.nper = len(row0)
        self.rows_end = int((row0 + nrows).max()) if self.nper else 0
        nret = np.maximum(nrows - 1, 0)
        off = np.concatenate([[0], np.cumsum(nret)[:-1]]) if self.nper else np.zeros(0, np.int64)
        self.total = int(nret.sum())
        dev = device or default_device()
        self.row0 = torch.as_tensor(row0.astype(np.int32), device=dev)
        self.nrows = torch.as_tensor(nrows.astype(np.int32), device=dev)
        self.off = torch.as_tensor(off.astype(np.int64), device=dev)
        self.ret_day = None
        if ret_day is not None:
            if len(ret_day) != self.total:
                raise ValueError("PeriodPlan: one calendar day per return")
            self.ret_day = torch.as_tensor(np.asarray(ret_day, dtype=np.int32), device=dev)


def simulate_periods(panel: torch.Tensor, W: torch.Tensor, plan, nrows=None, ret_day=None,
                     fc: float = 0.0, days_per_year: float = 252.0, rescale: bool = False,
                     want_end: bool = False):
    """Float each period's weights over its panel rows on the device (pq_simulate_periods;
    Strategy.simulate / floating_weights / Portfolio.turnover, src/portfolio.py:111-123,
    209-296).  ``panel`` (rows x n) and ``W`` (periods x n) are FP64 device tensors;
    ``plan`` is a PeriodPlan (or the row0 array, with ``nrows`` / ``ret_day`` given).
    Returns (ret [sum(nrows - 1)], wend [periods x n] or None, turnover [periods] or None),
    all on the device."""
    dev = panel.device
    nper, n = int(W.shape[0]), int(W.shape[1])
    if panel.dtype != F64 or W.dtype != F64 or panel.dim() != 2 or panel.shape[1] != n:
        raise ValueError("simulate_periods: FP64 panel (rows x n) and W (periods x n) expected")
    if not isinstance(plan, PeriodPlan):
        plan = PeriodPlan(plan, nrows, ret_day, dev, panel_rows=panel.shape[0])
    if plan.nper != nper or plan.rows_end > panel.shape[0]:
        raise ValueError("simulate_periods: plan does not match the weights / panel")
    if fc != 0.0 and plan.ret_day is None:
        raise ValueError("simulate_periods: fc needs one calendar day per return")
    if panel.stride(1) != 1:
        panel = panel.contiguous()
    if W.stride(1) != 1:
        W = W.contiguous()
    total = plan.total
    ret = torch.empty(max(total, 1), dtype=F64, device=dev)
    wend = torch.empty((nper, n), dtype=F64, device=dev) if want_end else None
    to = torch.empty(max(nper, 1), dtype=F64, device=dev) if want_end else None
    _lib.check(_lib.load().pq_simulate_periods(
        _ptr(panel), panel.stride(0), n, _ptr(W), W.stride(0), _ptr(plan.row0), _ptr(plan.nrows), nper,
        _ptr(plan.off), _ptr(plan.ret_day), float(fc), float(days_per_year), _ptr(ret), _ptr(wend),
        n, _ptr(to), int(bool(rescale)), _stream()), "pq_simulate_periods")
    return ret[:total], wend, (to[:nper] if to is not None else None)


# ----------------------------------------------------------------------------------------
# Quantile portfolios (PercentilePortfolios, src/optimization.py:356-417)
# ----------------------------------------------------------------------------------------

_PCT_PLANS: dict = {}


def percentile_plan(n: int, n_percentiles: int):
    """np.percentile's index plan for n values at linspace(0, 100, N + 1), with numpy's own
    arithmetic (numpy/lib/_function_base_impl.py: percentile, _quantile, _get_indexes,
    _get_gamma; method 'linear'): (prev int32 [N+1], next int32 [N+1], gamma float64 [N+1]).
    Threshold t interpolates the order statistics prev[t] and next[t] with weight gamma[t]."""
    n, N = int(n), int(n_percentiles)
    q = np.true_divide(np.linspace(0, 100, N + 1), np.float64(100))
    v = (n - 1) * q                               # virtual index
    prev = np.floor(v)
    nxt = prev + 1
    above = v >= n - 1                            # at the maximum: both indices are -1 (the last)
    prev[above] = -1
    nxt[above] = -1
    gamma = v - prev                              # _get_gamma sees the -1 (the two values are equal there)
    prev = prev.astype(np.intp) % n
    nxt = nxt.astype(np.intp) % n
    return prev.astype(np.int32), nxt.astype(np.int32), gamma.astype(np.float64)


def percentile_weights(scores: torch.Tensor, n_percentiles: int, sign: float = -1.0, n: int | None = None):
    """Quantile portfolios of every row of a device score panel (pq_percentile_batched;
    PercentilePortfolios.solve, src/optimization.py:398-417).  ``scores`` is an FP64 device
    tensor (B, n), or (B, ld) with ``n`` given (columns beyond n are never read); ``sign`` = -1
    ranks the raw scores as the reference does (its objective holds -scores).  Returns
    (w [B, n] long-short weights, bucket [B, n] int32 in 1..N, counts [B, N] int32,
    th [B, N+1] thresholds of sign * scores, status [B] int32: _lib.PQ_PCT_*), all on the
    device.  A row with an empty bucket or a NaN score has a non-OK status and NaN weights."""
    if scores.dim() != 2 or scores.dtype != F64 or not scores.is_cuda:
        raise ValueError("percentile_weights: FP64 device tensor (B, n) expected")
    B = int(scores.shape[0])
    n = int(scores.shape[1]) if n is None else int(n)
    N = int(n_percentiles)
    if not 1 <= n <= min(_lib.PQ_PCT_MAX_N, int(scores.shape[1])):
        raise ValueError(f"percentile_weights: n = {n} outside 1..{_lib.PQ_PCT_MAX_N} (the keys of one date are "
                         "sorted in LDS) or beyond the panel's columns")
    if not 1 <= N <= _lib.PQ_PCT_MAX_BUCKETS:
        raise ValueError(f"percentile_weights: n_percentiles = {N} outside 1..{_lib.PQ_PCT_MAX_BUCKETS}")
    if float(sign) not in (1.0, -1.0):
        raise ValueError("percentile_weights: sign must be +1 or -1")
    if scores.stride(1) != 1 or (B > 1 and scores.stride(0) < n):
        scores = scores.contiguous()
    lds = max(int(scores.stride(0)), n)           # (a one-row tensor may report any row stride)
    dev = scores.device
    plan = _PCT_PLANS.get((n, N, dev))
    if plan is None:
        plan = tuple(torch.from_numpy(a).to(dev) for a in percentile_plan(n, N))
        _PCT_PLANS[(n, N, dev)] = plan
    w = torch.empty((B, n), dtype=F64, device=dev)
    bucket = torch.empty((B, n), dtype=torch.int32, device=dev)
    counts = torch.empty((B, N), dtype=torch.int32, device=dev)
    th = torch.empty((B, N + 1), dtype=F64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    if B:
        _lib.check(_lib.load().pq_percentile_batched(
            _ptr(scores), lds, n, B, float(sign), N, _ptr(plan[0]), _ptr(plan[1]), _ptr(plan[2]),
            _ptr(th), _ptr(bucket), _ptr(counts), _ptr(w), _ptr(status), _stream()), "pq_percentile_batched")
    return w, bucket, counts, th, status


def _per_date(v, B: int, dev, what: str, who: str = "risk_parity_weights"):
    """A per-date FP64 device vector from a scalar or a (B,) tensor / array."""
    if isinstance(v, torch.Tensor):
        v = v.to(dev, dtype=F64).flatten()
    else:
        v = torch.as_tensor(np.asarray(v, dtype=np.float64), device=dev).flatten()
    if v.numel() == 1:
        v = v.expand(B)
    if v.numel() != B:
        raise ValueError(f"{who}: {what} must be a scalar or one value per date")
    return v.contiguous()


def risk_parity_weights(panel: "Panel", rows, tlen, budgets=None, a=None, c=None, centred: bool = True,
                        scale: float = 1.0, eps: float = 1e-10, max_sweeps: int = 500, moments=None):
    """Risk-parity (risk-budgeting) weights of every window (pq_risk_parity_batched): per date
    x = scale y* / sum(y*) with y* = argmin_{y > 0} 1/2 y' Sigma y - sum_i b_i log y_i, so that
    asset i carries the share b_i of the portfolio variance, on the window form
    Sigma = a Xc'Xc + c I (nothing n x n is formed).  ``rows`` / ``tlen``: the device row table
    (Panel.rows_to_device), at most 1024 rows per window.  ``budgets``: None (equal, 1/n), one
    (n,) row shared by all dates or (B, n); entries > 0, rows summing to 1 (the residual is
    relative to b_i).  ``a`` / ``c``: scalars or one value per date; defaults a = 1 / (T_d - 1) (the
    sample covariance; a one-row window has no sample covariance and is reported as bad input)
    and c = 0.  ``centred`` False: the uncentred Gram.  ``moments``: (mu, dg) of the windows where
    the caller already holds them (Panel.window_means / window_sumsq; mu None: uncentred), computed
    here otherwise.  Returns (x [B, n], stats [B, 4] = res,
    sweeps, x' Sigma x, sum(y), status [B] int32: _lib.PQ_RP_*), all on the device; a date whose
    status is PQ_RP_BAD_INPUT has NaN weights, one with PQ_RP_MAX_SWEEPS its last iterate and
    that iterate's residual.  Does not synchronise."""
    lib = _lib.load()
    B, tmax = int(rows.shape[0]), int(rows.shape[1])
    n, dev = panel.n, panel.device
    x = torch.empty((B, n), dtype=F64, device=dev)
    stats = torch.empty((B, 4), dtype=F64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return x, stats, status
    if not 1 <= tmax <= _lib.PQ_RP_TMAX:
        raise ValueError(f"risk_parity_weights: windows of up to {tmax} rows (supported: 1..{_lib.PQ_RP_TMAX})")
    rows = rows.contiguous()   # row pitch tmax, as every window entry point reads the table
    if budgets is None:
        bud = torch.full((1, n), 1.0 / n, dtype=F64, device=dev)
    else:
        bud = budgets if isinstance(budgets, torch.Tensor) else torch.as_tensor(np.asarray(budgets, dtype=np.float64))
        bud = bud.to(dev, dtype=F64).reshape(-1, n).contiguous()
        if bud.shape[0] not in (1, B):
            raise ValueError("risk_parity_weights: budgets must be (n,) or (B, n)")
    ldb = 0 if bud.shape[0] == 1 else n
    if a is None:
        a = 1.0 / (tlen.to(F64) - 1.0)
    a = _per_date(a, B, dev, "a")
    c = _per_date(0.0 if c is None else c, B, dev, "c")
    if moments is not None:
        mu, dg = moments
    else:
        mu = panel.window_means(rows, tlen) if centred else None
        dg = panel.window_sumsq(rows, tlen, mu)
    lr = LowRank(panel, rows, tlen, mu=mu, dg=dg).c_struct()
    _lib.check(lib.pq_risk_parity_batched(ctypes.byref(lr), n, B, _ptr(a), _ptr(c), _ptr(bud), ldb, float(scale),
                                          float(eps), int(max_sweeps), _ptr(x), x.stride(0), _ptr(stats),
                                          _ptr(status), _stream()), "pq_risk_parity_batched")
    return x, stats, status


HRP_CHUNK_BYTES = 2 << 30   # the dense covariance buffer of hrp_weights stays below this


def hrp_weights(panel: "Panel", rows, tlen, alpha=None, c=None, centred: bool = True, scale: float = 1.0,
                linkage: bool = False, chunk_bytes: int = HRP_CHUNK_BYTES, plan: "SlidePlan | None" = None,
                method: str = "single", dense=None):
    """Hierarchical-risk-parity weights of every window (pq_hrp_linkage_batched): per date the
    tree of the correlation distance of Sigma = alpha S + c I as SciPy's linkage builds it,
    its leaves in pre-order and the recursive bisection of that order by inverse-variance cluster
    variances; nothing is inverted or factored.  ``method``: 'single' (Prim's spanning tree, the
    default), 'complete', 'average', 'weighted' or 'ward' (the nearest-neighbour chain on a
    distance matrix in a second buffer of the chunk's size: ``chunk_bytes`` keeps sizing the
    covariance buffer alone, so that a launch still fills the CUs, and peak memory is then
    2 x ``chunk_bytes``); any other name raises ValueError.
    S is the window's sample covariance (Panel.cov mode 0, ddof = 1; ``centred`` False: the
    Gram X'X, mode 1), formed per chunk of dates so that
    the dense buffer stays under ``chunk_bytes``; one kernel launch per chunk.  ``alpha`` / ``c``:
    scalars or one value per date, defaults 1 and 0.  ``plan``: a SlidePlan of the row table where
    the caller has one (it covers the whole batch, so the batch has to fit one chunk).  ``dense``:
    a callable (rows_chunk, tlen_chunk, out) -> S that forms the chunk's dense matrices in place
    of Panel.cov (out: the first dates of the (per, ld, ld) buffer; the first n rows and columns
    of S are read, and a NaN there makes the date PQ_HRP_BAD_INPUT), e.g. the Gerber estimate;
    ``centred`` and ``plan`` are then unused.  At most
    _lib.PQ_HRP_NMAX assets.  Returns (x [B, n], order [B, n] int32, stats [B, 2] = x' Sigma x and
    the smallest gap between consecutive merge distances, status [B] int32: _lib.PQ_HRP_*), and
    with ``linkage`` also Z [B, n - 1, 4] in SciPy's layout, all on the device; a date whose
    status is PQ_HRP_BAD_INPUT (a one-row window, a zero-variance asset without a ridge,
    non-finite data) has NaN weights and order -1.  Does not synchronise."""
    lib = _lib.load()
    B, n, dev = int(rows.shape[0]), panel.n, panel.device
    if method not in _lib.HRP_METHODS:
        raise ValueError(f"hrp_weights: method '{method}' is not one of {', '.join(_lib.HRP_METHODS)}")
    meth = _lib.HRP_METHODS[method]
    if not 1 <= n <= _lib.PQ_HRP_NMAX:
        raise ValueError(f"hrp_weights: n = {n} outside 1..{_lib.PQ_HRP_NMAX} (the tree of one date lives in LDS)")
    x = torch.empty((B, n), dtype=F64, device=dev)
    order = torch.empty((B, n), dtype=torch.int32, device=dev)
    stats = torch.empty((B, 2), dtype=F64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    Z = torch.empty((B, n - 1, 4), dtype=F64, device=dev) if linkage else None
    out = (x, order, stats, status) + ((Z,) if linkage else ())
    if B == 0:
        return out
    rows = rows.contiguous()
    alpha = _per_date(1.0 if alpha is None else alpha, B, dev, "alpha", "hrp_weights")
    c = _per_date(0.0 if c is None else c, B, dev, "c", "hrp_weights")
    ld = round_up(n, 64)
    per = max(1, min(B, int(chunk_bytes) // (8 * ld * ld)))
    if plan is not None and per < B:
        raise ValueError("hrp_weights: a SlidePlan covers the whole batch; it needs chunk_bytes >= "
                         f"{8 * ld * ld * B} here")
    buf = torch.empty((per, ld, ld), dtype=F64, device=dev)
    # the distance matrices of a chunk: n rows of pitch ld per date (scratch)
    work = torch.empty((per, n, ld), dtype=F64, device=dev) if meth != _lib.PQ_HRP_SINGLE else None
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        if dense is not None:
            S = dense(rows[b0:b1], tlen[b0:b1], buf[:b1 - b0])
        else:
            S = panel.cov(rows[b0:b1], tlen[b0:b1], mode=0 if centred else 1, out=buf[:b1 - b0], plan=plan)
        _lib.check(lib.pq_hrp_linkage_batched(_ptr(S), ld, n, b1 - b0, _ptr(alpha[b0:]), _ptr(c[b0:]), float(scale),
                                              meth, None if work is None else _ptr(work), ld,
                                              _ptr(x[b0:]), x.stride(0), _ptr(order[b0:]), order.stride(0),
                                              _ptr(Z[b0:]) if linkage and n > 1 else None, _ptr(stats[b0:]),
                                              _ptr(status[b0:]), _stream()), "pq_hrp_linkage_batched")
    return out


GERBER_CHUNK_BYTES = 2 << 30   # the int8 sign panel of gerber_cov stays below this


def gerber_cov(panel: "Panel", rows, tlen, threshold: float = 0.5, variant: int = 2, corr: bool = False, out=None,
               chunk_bytes: int = GERBER_CHUNK_BYTES):
    """The Gerber covariance (Gerber et al. 2022) of every window (pq_gerber_cov_batched): per date
    the signs s_tk of the raw returns beyond ``threshold`` times the window's own standard
    deviation, the exact co-movement counts H = S'S on the int8 matrix cores, and
    Sigma_ij = g_ij sd_i sd_j with g_ij = H_ij / sqrt(a_i a_j) (``variant`` 2, positive
    semi-definite) or H_ij / (T - N^NN_ij) (``variant`` 1); ``corr``: g itself.  ``rows`` / ``tlen``:
    the device row table, at most _lib.PQ_GERBER_TMAX rows per window.  ``out``: a (B, ld, ld)
    buffer, ld = round_up(n, 64), of which only [0, n) x [0, n) of every date is written (None: a
    zero-filled one is allocated).  The int8 sign panel is scratch, allocated per chunk of dates so
    that it stays under ``chunk_bytes``.  Returns (S [B, ld, ld], status [B] int32: _lib.PQ_GERBER_*,
    counts [B, ld] int32: a_k), on the device; a PQ_GERBER_BAD_INPUT date (fewer than 2 rows, a
    non-finite value, a constant column, an asset that never moves beyond its threshold) has a NaN
    block.  Does not synchronise."""
    lib = _lib.load()
    from .covariance import _gerber_check
    threshold, variant = _gerber_check(threshold, variant)
    B, tmax = int(rows.shape[0]), int(rows.shape[1])
    n, dev = panel.n, panel.device
    ld = round_up(n, 64)
    if not 1 <= tmax <= _lib.PQ_GERBER_TMAX:
        raise ValueError(f"gerber_cov: windows of up to {tmax} rows (supported: 1..{_lib.PQ_GERBER_TMAX})")
    if out is None:
        out = torch.zeros((B, ld, ld), dtype=F64, device=dev)
    elif tuple(out.shape) != (B, ld, ld) or out.dtype != F64 or not out.is_contiguous():
        raise ValueError(f"gerber_cov: out must be a contiguous float64 ({B}, {ld}, {ld}) tensor")
    status = torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty((B, ld), dtype=torch.int32, device=dev)
    if B == 0:
        return out, status, counts
    rows = rows.contiguous()
    per_date = ld * round_up(tmax, 64)   # bytes of a date's sign panel
    per = max(1, min(B, int(chunk_bytes) // per_date))
    St = torch.empty((per, per_date), dtype=torch.int8, device=dev)
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        r, t = rows[b0:b1], tlen[b0:b1]
        dg = panel.window_sumsq(r, t, panel.window_means(r, t))
        _lib.check(lib.pq_gerber_cov_batched(_ptr(panel.R), panel.R.stride(0), n, _ptr(r), _ptr(t), tmax, b1 - b0,
                                             _ptr(dg), dg.stride(0), threshold, variant, int(bool(corr)),
                                             _lib.PQ_GERBER_SIGNS | _lib.PQ_GERBER_GRAM, _ptr(St),
                                             _ptr(counts[b0:]), counts.stride(0), _ptr(out[b0:]), ld, out.stride(0),
                                             _ptr(status[b0:]), _stream()), "pq_gerber_cov_batched")
    return out, status, counts


RANK_CHUNK_BYTES = 2 << 30   # the rank scratch of rank_cov stays below this
RANK_KINDS = {"spearman": _lib.PQ_RANK_SPEARMAN, "kendall": _lib.PQ_RANK_KENDALL}
RANK_OUTPUTS = {"cov": _lib.PQ_RANK_COV, "corr": _lib.PQ_RANK_CORR, "counts": _lib.PQ_RANK_COUNTS}


def rank_cov(panel: "Panel", rows, tlen, kind: str = "spearman", output: str = "cov", out=None,
             chunk_bytes: int = RANK_CHUNK_BYTES):
    """The rank covariance of every window (pq_rank_cov_batched): Spearman's rho (``kind``
    'spearman') or Kendall's tau-b ('kendall') of the window's columns as the correlation g, and
    Sigma_ij = g_ij sd_i sd_j with the window's own standard deviations (``output`` 'cov'); 'corr':
    g itself; 'counts': the exact integer numerator as doubles -- C = c'c of the centred doubled
    mid-ranks (Spearman), H = concordant minus discordant pairs of days (Kendall).  Spearman: the
    ranking kernel writes the rank panel, Panel.cov(mode=1) forms its Gram per date on the FP64
    matrix cores, an epilogue kernel finishes in place; Kendall: the ranking kernel writes int16
    ranks and the Gram kernel builds the signs of the T (T - 1) / 2 day pairs on the fly for the
    int8 matrix cores.  ``rows`` / ``tlen``: the device row table, at most _lib.PQ_RANK_TMAX rows
    per window.  ``out``: a (B, ld, ld) buffer, ld = round_up(n, 64): [0, n) x [0, n) of every date
    carries the result and the padding is set to zero (None: a buffer is allocated).  The rank
    panels are scratch, allocated per chunk of dates so that they stay under ``chunk_bytes``; the
    results do not depend on the chunking.  Returns (S [B, ld, ld], status [B] int32:
    _lib.PQ_RANK_*, diag [B, ld] float64: C_kk or H_kk, exact), on the device; a PQ_RANK_BAD_INPUT
    date (fewer than 2 rows, a non-finite value, a constant column) has a NaN block.  ValueError
    for an unknown kind or output, a wrong ``out`` or a window length outside 1.._lib.PQ_RANK_TMAX,
    before anything runs.  Does not synchronise."""
    lib = _lib.load()
    if kind not in RANK_KINDS:
        raise ValueError(f"rank_cov: kind = {kind!r} is not one of {sorted(RANK_KINDS)}")
    if output not in RANK_OUTPUTS:
        raise ValueError(f"rank_cov: output = {output!r} is not one of {sorted(RANK_OUTPUTS)}")
    B, tmax = int(rows.shape[0]), int(rows.shape[1])
    n, dev = panel.n, panel.device
    ld = round_up(n, 64)
    if not 1 <= tmax <= _lib.PQ_RANK_TMAX:
        raise ValueError(f"rank_cov: windows of up to {tmax} rows (supported: 1..{_lib.PQ_RANK_TMAX})")
    if out is None:
        out = torch.empty((B, ld, ld), dtype=F64, device=dev)
    elif tuple(out.shape) != (B, ld, ld) or out.dtype != F64 or not out.is_contiguous():
        raise ValueError(f"rank_cov: out must be a contiguous float64 ({B}, {ld}, {ld}) tensor")
    status = torch.empty(B, dtype=torch.int32, device=dev)
    diag = torch.empty((B, ld), dtype=F64, device=dev)
    if B == 0:
        return out, status, diag
    rows = rows.contiguous()
    kd, mode = RANK_KINDS[kind], RANK_OUTPUTS[output]
    spearman = kd == _lib.PQ_RANK_SPEARMAN
    per_date = 8 * tmax * n if spearman else 2 * ld * round_up(tmax, 64)   # bytes of a date's rank panel
    per = max(1, min(B, int(chunk_bytes) // per_date))
    if spearman:   # date b of a chunk is the rows [b tmax, (b + 1) tmax) of the scratch panel
        scratch = torch.empty((per * tmax, n), dtype=F64, device=dev)
        ranks = Panel(scratch, device=dev)
        rrows = torch.arange(per * tmax, dtype=torch.int32, device=dev).view(per, tmax)
        rlen = torch.full((per,), tmax, dtype=torch.int32, device=dev)   # the rows past a window are zero
    else:
        scratch = torch.empty((per, per_date // 2), dtype=torch.int16, device=dev)

    def call(b0, b1, r, t, dg, stages):
        _lib.check(lib.pq_rank_cov_batched(_ptr(panel.R), panel.R.stride(0), n, _ptr(r), _ptr(t), tmax, b1 - b0,
                                           _ptr(dg), dg.stride(0), kd, mode, stages, _ptr(scratch), n,
                                           _ptr(diag[b0:]), diag.stride(0), _ptr(out[b0:]), ld, out.stride(0),
                                           _ptr(status[b0:]), _stream()), "pq_rank_cov_batched")
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        r, t = rows[b0:b1], tlen[b0:b1]
        dg = panel.window_sumsq(r, t, panel.window_means(r, t))
        if spearman:
            call(b0, b1, r, t, dg, _lib.PQ_RANK_RANKS)
            ranks.cov(rrows[:b1 - b0], rlen[:b1 - b0], mode=1, out=out[b0:b1])
            call(b0, b1, r, t, dg, _lib.PQ_RANK_FINISH)
        else:
            call(b0, b1, r, t, dg, _lib.PQ_RANK_RANKS | _lib.PQ_RANK_FINISH)
    return out, status, diag


def ewma_age_weights(tmax: int, halflife=None, decay=None) -> np.ndarray:
    """The age table of the exponentially weighted covariance, ``tmax + 1`` doubles built with NumPy
    on the host (and only here, so that the kernels and a host model use the same bits):
    wage[k] = 0.5 ** (k / halflife), or decay ** k; the spec is checked by covariance._ewma_check."""
    from .covariance import _ewma_check
    halflife, decay = _ewma_check(halflife, decay)
    k = np.arange(int(tmax) + 1, dtype=np.float64)
    if halflife is not None:
        return np.power(0.5, k / halflife)
    return np.power(decay, k)


def ewma_cov(panel: "Panel", rows, tlen, halflife=None, decay=None, plan: "SlidePlan | None" = None, out=None):
    """The exponentially weighted covariance (RiskMetrics 1996) of every window
    (pq_ewma_cov_batched), with NumPy's and pandas' definition: a row of age k (the newest row of
    a window has age 0) weighs w = 0.5 ** (k / halflife), or decay ** k,
    Sigma = sum w (x - m)(x - m)' / (W1 - W2 / W1) with the weighted mean m, W1 = sum w and
    W2 = sum w^2 -- np.cov(aweights=w), the last block of ewm(adjust=True).cov(bias=False).  One of
    ``halflife`` (rows, > 0, inf allowed) and ``decay`` (0 < decay <= 1) may be given, neither means
    decay = 0.94; halflife = inf or decay = 1 is the ddof = 1 sample covariance.  ``rows`` /
    ``tlen``: the device row table, at most _lib.PQ_EWMA_TMAX rows per window.  ``plan``: a SlidePlan
    of the same table; overlapping windows are then formed by the decaying rank-2s recursion
    instead of a weighted SYRK per date (the same estimate to rounding).  ``out``: a (B, ld, ld)
    buffer, ld = round_up(n, 64): [0, n) x [0, n) of every date carries the result, symmetric bit
    for bit, and the padding is set to zero (None: a buffer is allocated).  Returns (S [B, ld, ld],
    status [B] int32: _lib.PQ_EWMA_*, mean [B, ld] float64: the weighted means), on the device; a
    PQ_EWMA_BAD_INPUT date (fewer than 2 rows, a non-finite value, a decay so fast that
    W1 - W2 / W1 is not positive) has a NaN block and affects no other date.  ValueError for a bad
    spec, a wrong ``out`` or a window length outside 1.._lib.PQ_EWMA_TMAX, before anything runs.
    Does not synchronise."""
    B, tmax = int(rows.shape[0]), int(rows.shape[1])
    wage = ewma_age_weights(tmax, halflife, decay)
    lib = _lib.load()
    n, dev = panel.n, panel.device
    ld = round_up(n, 64)
    if not 1 <= tmax <= _lib.PQ_EWMA_TMAX:
        raise ValueError(f"ewma_cov: windows of up to {tmax} rows (supported: 1..{_lib.PQ_EWMA_TMAX})")
    if out is None:
        out = torch.empty((B, ld, ld), dtype=F64, device=dev)
    elif tuple(out.shape) != (B, ld, ld) or out.dtype != F64 or not out.is_contiguous():
        raise ValueError(f"ewma_cov: out must be a contiguous float64 ({B}, {ld}, {ld}) tensor")
    status = torch.empty(B, dtype=torch.int32, device=dev)
    mean = torch.empty((B, ld), dtype=F64, device=dev)
    if B == 0:
        return out, status, mean
    rows = rows.contiguous()
    wdev = torch.from_numpy(wage).to(dev)
    wsqrt = torch.empty_like(wdev)   # scratch: the square roots of the table
    wsum = torch.empty((B, 2), dtype=F64, device=dev)
    slide = plan is not None
    _lib.check(lib.pq_ewma_cov_batched(_ptr(panel.R), panel.R.stride(0), n, _ptr(rows), _ptr(tlen), tmax, B,
                                       _ptr(wdev), _ptr(wsqrt), _ptr(mean), mean.stride(0), _ptr(wsum), _ptr(out), ld,
                                       out.stride(0), _ptr(status), _ptr(plan.gstart) if slide else None,
                                       plan.ngroups if slide else 0, _ptr(plan.shift) if slide else None,
                                       _stream()), "pq_ewma_cov_batched")
    return out, status, mean


PCA_CHUNK_BYTES = 2 << 30   # Gram, eigenvector and work buffers of pca_window_form stay below this
# the eigensolver of pca_window_form where the caller names none: on the 4749 window Grams of config 3
# (252 x 252) rocSOLVER's eigh takes 432 ms, the block-Jacobi kernels 2994 ms (profiles/pca_cov_bench.log)
PCA_BACKEND = "rocsolver"


class PcaWindowForm:
    """The PCA factor covariance of every date as an uncentred window form: Sigma_b = Z_b'Z_b +
    sigma2[b] I with Z_b the rows ``rows[b, :tlen[b]]`` of ``panel`` (engine.pca_window_form)."""

    def __init__(self, panel, rows, tlen, sigma2, evals, status):
        self.panel, self.rows, self.tlen = panel, rows, tlen
        self.sigma2, self.evals, self.status = sigma2, evals, status

    def dense(self, i: int) -> torch.Tensor:
        """The n x n Sigma of date i (torch, on the device; NaN for a PQ_PCA_BAD_INPUT date)."""
        Z = self.panel.R[self.rows[i, :int(self.tlen[i].item())].long()]
        return Z.T @ Z + self.sigma2[i] * torch.eye(self.panel.n, dtype=F64, device=Z.device)


def _row_sums_fixed(x: torch.Tensor) -> torch.Tensor:
    """Row sums of a (B, m) tensor by a fixed binary tree of elementwise additions: a row's bits
    do not depend on the other rows of the batch (torch.sum chooses its reduction by the shape)."""
    W = 1 << max(0, int(x.shape[1]) - 1).bit_length()
    if W != x.shape[1]:
        x = torch.cat([x, x.new_zeros((x.shape[0], W - x.shape[1]))], 1)
    while W > 1:
        W //= 2
        x = x[:, :W] + x[:, W:2 * W]
    return x[:, 0]


def _pca_eigen_map(ev, dg, tlen, n: int, kcap: int, mp: bool, finite):
    """The eigenvalue map of pca_window_form on one chunk: from the unsorted Gram eigenvalues
    ``ev`` (Bc, >= 1), diag(Xc'Xc) ``dg`` (Bc, n) and the window lengths, per date the factor
    count, the noise level, l_1..l_kcap, the row scales s, the eigenvector columns and the OK
    flag.  Sorting, elementwise operations and fixed-order sums only, so that a date's result does
    not depend on the batch it is in."""
    dev = ev.device
    ssq = _row_sums_fixed(dg)
    Tf = tlen.to(F64)
    dof = Tf - 1.0
    g, idx = torch.sort(ev, dim=1, descending=True)
    W = kcap + 1
    if g.shape[1] < W:   # l_j = 0 beyond the Gram's size
        pad = W - g.shape[1]
        g = torch.cat([g, torch.zeros((g.shape[0], pad), dtype=F64, device=dev)], 1)
        idx = torch.cat([idx, torch.zeros((idx.shape[0], pad), dtype=idx.dtype, device=dev)], 1)
    g, idx = g[:, :W], idx[:, :W]
    l = g / dof[:, None]
    ks = torch.arange(1, kcap + 1, device=dev)
    cs = torch.empty((ev.shape[0], kcap), dtype=F64, device=dev)
    acc = torch.zeros(ev.shape[0], dtype=F64, device=dev)
    for j in range(kcap):   # (the running sum l_1 + .. + l_j in a fixed order; kcap <= PQ_PCA_KMAX)
        acc = acc + l[:, j]
        cs[:, j] = acc
    sig_all = ((ssq / dof)[:, None] - cs) / (n - ks).to(F64)   # sigma2 with k kept
    if mp:   # the smallest k whose next eigenvalue lies inside the Marchenko-Pastur bulk of its noise level
        edge = (1.0 + torch.sqrt(n / Tf)) ** 2
        hit = l[:, 1:W] <= edge[:, None] * sig_all
        k_b = torch.where(hit.any(1), torch.argmax(hit.to(torch.int32), 1) + 1, kcap)
    else:
        k_b = torch.full((ev.shape[0],), kcap, dtype=torch.int64, device=dev)
    sel = (k_b - 1)[:, None]
    sig = sig_all.gather(1, sel).squeeze(1)
    gk = g.gather(1, sel).squeeze(1)
    ok = finite & (tlen >= 2) & (gk > Tf * 2.0 ** -52 * g[:, 0]) & (sig > 0) & torch.isfinite(sig)
    used = (ks[None, :] <= k_b[:, None]) & ok[:, None]
    lk = l[:, :kcap]
    s = torch.sqrt(torch.clamp(1.0 - sig[:, None] / lk, min=0.0) / dof[:, None])
    s = torch.where(used, s, torch.zeros_like(s)).contiguous()
    nan = torch.full_like(sig, float("nan"))
    evals = torch.where(used, lk, torch.zeros_like(lk))
    evals = torch.where(ok[:, None], evals, nan[:, None])
    kcnt = torch.where(ok, k_b, torch.zeros_like(k_b)).to(torch.int32)
    return kcnt, torch.where(ok, sig, nan), evals, s, idx[:, :kcap].to(torch.int32).contiguous(), ok


def pca_window_form(panel: "Panel", rows, tlen, n_factors="mp", backend: str | None = None, kmax: int = 64,
                    chunk_bytes: int = PCA_CHUNK_BYTES) -> PcaWindowForm:
    """The PCA factor covariance (probabilistic PCA, Tipping & Bishop; sklearn's
    PCA.get_covariance()) of every window as a k-row window form.  With G = Xc Xc' = V diag(g) V'
    the T x T Gram of the centred window, l_j = g_j / (T - 1) and tr S from Panel.window_sumsq,
        sigma2 = (tr S - sum_{j<=k} l_j) / (n - k),    Z_j = sqrt((1 - sigma2 / l_j) / (T - 1)) v_j' Xc,
        Sigma = Z'Z + sigma2 I:
    the k largest principal components kept, the rest of the spectrum replaced by one noise level
    that preserves the trace.  Z is written as k rows of a factor panel, so that
    risk_parity_weights(form.panel, form.rows, form.tlen, centred=False, a=1, c=form.sigma2) and
    hrp_weights(..., centred=False, alpha=1, c=form.sigma2) solve on Sigma as they stand.

    ``n_factors``: an int k with 1 <= k <= min(kmax, n - 1), or 'mp': per date the smallest k in
    1..kmax with l_{k+1} <= (1 + sqrt(n / T))^2 sigma2_k (the next eigenvalue inside the
    Marchenko-Pastur bulk of the noise level with k kept; l_j = 0 beyond the Gram's size), kmax
    where none is.  ``kmax`` <= _lib.PQ_PCA_KMAX.  ``backend``: 'jacobi' (helper_functions.sym_eig)
    or 'rocsolver' (torch.linalg.eigh); None: PCA_BACKEND.  Per chunk of dates (Gram, eigenvectors
    and solver work below ``chunk_bytes``): window means, pq_window_gram_batched, the
    eigendecomposition, the eigenvalue map in a few O(T) device ops, pq_window_project_batched.

    Returns a PcaWindowForm: ``panel`` (the factor rows), ``rows`` (B, kmax_used) int32, ``tlen``
    (B,) int32 the factor count k_b, ``sigma2`` (B,), ``evals`` (B, kmax_used) the l_j kept (0
    beyond k_b), ``status`` (B,) int32.  A date is _lib.PQ_PCA_BAD_INPUT where tlen < 2, the Gram
    is not finite, g_k <= T 2^-52 g_1 (more factors than the window has rank) or sigma2 <= 0: its
    sigma2 and evals are NaN and it has no factor rows (k_b = 0), so the consumers report it as
    their own bad input; its neighbours are unaffected.  Synchronises (the size of the factor
    panel is read back per chunk)."""
    from .helper_functions import sym_eig
    lib = _lib.load()
    B, tmax = int(rows.shape[0]), int(rows.shape[1])
    n, dev = panel.n, panel.device
    backend = PCA_BACKEND if backend is None else backend
    if backend not in ("jacobi", "rocsolver"):
        raise ValueError("pca_window_form: backend must be 'jacobi' or 'rocsolver'")
    if isinstance(kmax, bool) or not isinstance(kmax, (int, np.integer)) or not 1 <= kmax <= _lib.PQ_PCA_KMAX:
        raise ValueError(f"pca_window_form: kmax = {kmax} outside 1..{_lib.PQ_PCA_KMAX}")
    if n < 2:
        raise ValueError("pca_window_form: a factor model needs at least 2 assets")
    kcap = min(int(kmax), n - 1)
    mp = isinstance(n_factors, str) and n_factors == "mp"
    if not mp:
        if (isinstance(n_factors, bool) or not isinstance(n_factors, (int, np.integer))
                or not 1 <= n_factors <= kcap):
            raise ValueError(f"pca_window_form: n_factors = {n_factors!r} must be 'mp' or an int in "
                             f"1..min(kmax, n - 1) = {kcap}")
        kcap = int(n_factors)
    if not 1 <= tmax <= _lib.PQ_PCA_TMAX:
        raise ValueError(f"pca_window_form: windows of up to {tmax} rows (supported: 1..{_lib.PQ_PCA_TMAX})")
    rows = rows.contiguous()
    ldg = round_up(tmax, 64)
    work = int(lib.pq_sym_eig_work_doubles(ldg)) if backend == "jacobi" else 2 * ldg * ldg
    per = max(1, min(B, int(chunk_bytes) // (8 * (2 * ldg * ldg + work))))
    sigma2 = torch.empty(B, dtype=F64, device=dev)
    evals = torch.empty((B, kcap), dtype=F64, device=dev)
    kcnt = torch.empty(B, dtype=torch.int32, device=dev)
    frow = torch.empty(B, dtype=torch.int32, device=dev)
    G = torch.empty((min(per, B), ldg, ldg), dtype=F64, device=dev)
    pieces, base = [], 0
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        r, t = rows[b0:b1], tlen[b0:b1]
        mu = panel.window_means(r, t)
        dg = panel.window_sumsq(r, t, mu)
        Gc = G[:b1 - b0]
        _lib.check(lib.pq_window_gram_batched(_ptr(panel.R), panel.R.stride(0), n, _ptr(r), _ptr(t), tmax, b1 - b0,
                                              _ptr(mu), mu.stride(0), _ptr(Gc), ldg, ldg * ldg, _stream()),
                   "pq_window_gram_batched")
        # a NaN or inf in the window (or in its mean) reaches the Gram's diagonal: such a date is
        # bad input, and the eigensolver sees a zero matrix in its place
        finite = torch.isfinite(torch.diagonal(Gc, dim1=1, dim2=2)).all(1)
        Gc.masked_fill_(~finite[:, None, None], 0.0)
        if backend == "jacobi":
            ev, V = sym_eig(Gc, tmax)
            ev, ldv = ev[:, :tmax], ldg
        else:
            ev, V = torch.linalg.eigh(Gc[:, :tmax, :tmax])
            V, ldv = V.contiguous(), tmax
        kc, sig, lk, s, col, _ = _pca_eigen_map(ev, dg[:, :n], t, n, kcap, mp, finite)
        fr = (torch.cumsum(kc, 0, dtype=torch.int64) - kc).to(torch.int32)   # first factor row inside the chunk
        total = int(kc.sum().item())
        sigma2[b0:b1], evals[b0:b1], kcnt[b0:b1], frow[b0:b1] = sig, lk, kc, fr + base
        if total:
            F = torch.empty((total, n), dtype=F64, device=dev)
            _lib.check(lib.pq_window_project_batched(_ptr(panel.R), panel.R.stride(0), n, _ptr(r), _ptr(t), tmax,
                                                     b1 - b0, _ptr(mu), mu.stride(0), _ptr(V), ldv, ldv * ldv,
                                                     _ptr(col), _ptr(s), _ptr(kc), kcap,
                                                     _ptr(fr), _ptr(F), n, _stream()),
                       "pq_window_project_batched")
            pieces.append(F)
            base += total
    used = max(1, int(kcnt.max().item())) if B else 1
    F = torch.cat(pieces) if len(pieces) > 1 else pieces[0] if pieces else torch.zeros((1, n), dtype=F64, device=dev)
    j = torch.arange(used, dtype=torch.int32, device=dev)[None, :]
    frows = torch.where(j < kcnt[:, None], frow[:, None] + j, torch.zeros_like(j)).contiguous()
    status = torch.where(kcnt > 0, _lib.PQ_PCA_OK, _lib.PQ_PCA_BAD_INPUT).to(torch.int32)
    return PcaWindowForm(Panel(F, device=dev), frows, kcnt, sigma2, evals[:, :used].contiguous(), status)
