# Host-side API restatement of PorQua (part of the GeomScale project; reference tree
# amolrpatil21/PorQua): src/optimization.py.  PorQua is Copyright (c) 2024 Cyril Bachelard and
# Minh Ha Ho and licensed under the GNU LGPL v3; this module keeps that API and its
# behaviour (quirks included) so that the MI355X engine is a drop-in, and is distributed
# under the same licence terms.
"""Optimization classes (mirror of the hot-path part of src/optimization.py:40-259).

Each class keeps the reference API (``set_objective(optimization_data)``, ``solve()``,
``model_qpsolvers()``, ``results``) and adds a batched objective builder used by the
batched backtest: ``objective_batch(stage)`` returns the device-resident P (as the K1
output plus a per-date scale / diagonal term), q and the constant for every date at once.

Deliberate differences from the reference ("Reference defects"):
* ``OptimizationParameter`` defaults ``solver_name`` to 'mi355x' (the engine of this
  package) and lets ``verbose=False`` stick (src/optimization.py:45-46).
* ``MeanVariance`` uses the mean estimator that is passed in; the reference stores the
  class instead of the instance (src/optimization.py:165).
* ``PercentilePortfolios`` leaves out the reference's unseeded noise on exact-zero scores
  (src/optimization.py:393); zero weights are +0.0.
LAD runs on the batched device IPM of porqua_amd/lad.py; PercentilePortfolios (ranking, not
the QP path) runs on the batched order-statistics kernel (pq_percentile_batched), one date
in ``solve()`` and every date of a backtest through ``percentile_batch``.  RiskParity (beyond the
reference: risk budgeting is not a QP) runs on the batched coordinate-descent kernel
(pq_risk_parity_batched), one date in ``solve()`` and every date through ``risk_parity_batch``;
HierarchicalRiskParity on the batched tree-and-bisection kernel (pq_hrp_batched), through
``hrp_batch``.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Optional

import numpy as np
import pandas as pd

from . import qp_problems
from .constraints import Constraints
from .covariance import DENSE_ONLY_METHODS, RANK_METHODS, Covariance
from .helper_functions import to_numpy
from .mean_estimation import MeanEstimator
from .optimization_data import OptimizationData


class OptimizationParameter(dict):

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.__dict__ = self
        if not self.get("solver_name"):
            self["solver_name"] = qp_problems.ENGINE_SOLVER
        self.setdefault("verbose", True)
        self.setdefault("allow_suboptimal", False)


class Objective(dict):
    pass


def _device_gram(X, y=None):
    """(X'X, X'y, y'y) of one window on the device (K1 Gram mode + pq_gram_xy)."""
    from . import engine
    Xv = np.ascontiguousarray(to_numpy(X), dtype=np.float64)
    T, n = Xv.shape
    yv = None if y is None else np.ascontiguousarray(to_numpy(y), dtype=np.float64).reshape(-1)
    pan = engine.Panel(Xv, yv)
    rows, tlen = pan.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
    G = pan.cov(rows, tlen, mode=1)[0, :n, :n].cpu().numpy()
    if yv is None:
        return G, None, None
    xty, yty = pan.gram_xy(rows, tlen)
    return G, xty[0, :n].cpu().numpy(), float(yty[0].item())


class Optimization(ABC):

    def __init__(self, params: OptimizationParameter = None, constraints: Constraints = None, **kwargs):
        self.params = OptimizationParameter(**kwargs) if params is None else params
        self.objective = Objective()
        self.constraints = Constraints() if constraints is None else constraints
        self.model = None
        self.results = None

    @abstractmethod
    def set_objective(self, optimization_data: OptimizationData) -> None:
        raise NotImplementedError("Method 'set_objective' must be implemented in derived class.")

    def objective_batch(self, stage):
        """Batched objective for the device backtest; ``None`` = not batchable."""
        return None

    def solve(self) -> bool:
        """src/optimization.py:72-75 (subclasses in the reference only forward here)."""
        self.solve_qpsolvers()
        return self.results["status"]

    def solve_qpsolvers(self) -> None:
        self.model_qpsolvers()
        self.model.solve()
        universe = self.constraints.selection
        sol = self.model["solution"]
        w = sol.x[:len(universe)] if sol.found else [None] * len(universe)
        self.results = {"weights": pd.Series(w, index=universe).to_dict(), "status": sol.found}

    def model_qpsolvers(self) -> None:
        """Assemble the QuadraticProgram exactly as src/optimization.py:91-143."""
        if "P" not in self.objective:
            raise ValueError("Missing matrix 'P' in objective.")
        P = to_numpy(self.objective["P"])
        q = to_numpy(self.objective["q"]) if "q" in self.objective else np.zeros(len(self.constraints.selection))
        self.objective["P"], self.objective["q"] = P, q
        universe = self.constraints.selection
        GhAb = self.constraints.to_GhAb()
        boxed = self.constraints.box["box_type"] != "NA"
        lb = self.constraints.box["lower"].to_numpy() if boxed else None
        ub = self.constraints.box["upper"].to_numpy() if boxed else None
        self.model = qp_problems.QuadraticProgram(P=P, q=q, constant=self.objective.get("constant"),
                                                  G=GhAb["G"], h=GhAb["h"], A=GhAb["A"], b=GhAb["b"],
                                                  lb=lb, ub=ub, params=self.params)
        tocon = self.constraints.l1.get("turnover")
        x0 = tocon["x0"] if tocon is not None and tocon.get("x0") is not None else self.params.get("x0")
        x_init = {a: x0.get(a, 0) for a in universe} if x0 is not None else None
        tc = self.params.get("transaction_cost")
        if tc is not None and x_init is not None:
            self.model.linearize_turnover_objective(pd.Series(x_init), tc)
        if tocon and not tc and x_init is not None:
            self.model.linearize_turnover_constraint(pd.Series(x_init), tocon["rhs"])
        levcon = self.constraints.l1.get("leverage")
        if levcon is not None:
            self.model.linearize_leverage_constraint(N=len(universe), leverage_budget=levcon["rhs"])


class EmptyOptimization(Optimization):

    def set_objective(self, optimization_data=None) -> None:
        pass

    def solve(self) -> bool:
        return super().solve()


class MeanVariance(Optimization):
    """P = 2 * risk_aversion * Sigma, q = -mu_geometric (src/optimization.py:157-177).

    With the 'pca' covariance ``set_objective`` takes the dense estimate of
    ``Covariance.estimate`` and ``objective_batch`` returns None, so a backtest runs the serial
    loop.  The QP window path on the factor form is deliberately not offered: its capacitance
    would be k + mg wide, and the backtest's group plan is built from the original row table,
    which must not be mixed with the factor rows.

    With the 'gerber' covariance, variant 2 (positive semi-definite by construction) takes the dense
    batched route whatever ``prefer_lowrank`` says -- its thresholds are per date, so there is no
    window form --; variant 1 can be indefinite, so ``objective_batch`` returns None and the serial
    loop lets ``Covariance.estimate`` check and repair every date.  'spearman' and 'kendall' are
    positive semi-definite by construction and take the dense batched route in the same way
    (covariance.DENSE_ONLY_METHODS names the methods without a window form).  'ewma' is one of them,
    positive semi-definite by construction too, and the only one whose estimator takes the stage's
    slide plan: the consecutive windows of a daily backtest are formed by the decaying recursion of
    engine.ewma_cov."""

    batch_handles_nan = True   # windows with gaps: pairwise covariance + skipna means, batched

    def __init__(self, covariance: Optional[Covariance] = None,
                 mean_estimator: Optional[MeanEstimator] = None, **kwargs):
        super().__init__(**kwargs)
        self.covariance = Covariance() if covariance is None else covariance
        self.mean_estimator = MeanEstimator() if mean_estimator is None else mean_estimator
        self.params.setdefault("risk_aversion", 1)

    def set_objective(self, optimization_data: OptimizationData) -> None:
        X = optimization_data["return_series"]
        covmat = self.covariance.estimate(X=X) * self.params["risk_aversion"] * 2
        mu = self.mean_estimator.estimate(X=X) * (-1)
        self.objective = Objective(q=mu, P=covmat)

    def objective_batch(self, stage):
        import torch
        from . import engine
        if self.covariance.spec["method"] == "pca":   # the dense estimate, date by date
            return None
        method = self.covariance.spec["method"]
        dense_only = method in DENSE_ONLY_METHODS   # estimated per date from its own window: no window form
        if method == "gerber" and self.covariance.gerber_spec[1] != 2:   # variant 1 can be indefinite: the checked serial loop
            return None
        nan = stage.panel.has_nan   # missing values: pairwise covariance, dense P (no window form)
        lowrank = stage.prefer_lowrank and method != "duv" and not nan and not dense_only
        # (the dense-only estimators read each date's own window; 'ewma' alone has a sliding form)
        no_plan = nan or lowrank or (dense_only and method != "ewma")
        S, pdiag, mu_c, dg = self.covariance.estimate_batch_lr(
            stage.panel, stage.rows, stage.tlen, out=None if lowrank else stage.P_buffer(),
            plan=None if no_plan else stage.slide_plan(), materialise=not lowrank,
            groups=stage.group_plan() if lowrank else None)
        ra = float(self.params["risk_aversion"])
        B = stage.batch
        dev = stage.device
        if (nan or dense_only) and S is None:
            return None
        # 'ledoit_wolf' / 'oas': Sigma* = (1 - delta) S + pdiag I with a per-date delta; the
        # factor (1 - delta) goes into w_scale (window form) or the returned scale (dense)
        delta = getattr(self.covariance, "shrinkage_batch_", None)
        if mu_c is None and not nan and not dense_only:  # duv: identity covariance
            S = stage.identity_P()
            pdiag = torch.zeros(B, dtype=torch.float64, device=dev)
        elif lowrank:   # factored form S = Xc'Xc / (T - 1) for the Woodbury solver (no n x n S)
            stage.lowrank = engine.LowRank(stage.panel, stage.rows, stage.tlen, mu=mu_c,
                                           w_scale=(1.0 if delta is None else 1.0 - delta)
                                           / (stage.tlen.to(torch.float64) - 1.0), dg=dg)
        me = self.mean_estimator
        if me.spec.get("method") != "geometric":
            return None
        a, b = me.window(int(stage.tlen_host.max()))
        if not np.all(stage.tlen_host == stage.tlen_host[0]) and (a, b) != (0, int(stage.tlen_host[0])):
            return None
        mrows, mtlen = stage.sub_windows(a, b)
        if nan:
            mu = stage.panel.window_nanmeans(mrows, mtlen, geometric=True)
            if bool(torch.isnan(mu[:, :stage.n]).any().item()):
                return None
        elif lowrank and mrows is stage.rows and stage.group_plan().ok:
            # the full windows of slide groups: one sliding log-sum pass per group
            mu = stage.panel.window_geomeans_grouped(stage.group_plan(), stage.tlen)
        else:
            mu = stage.panel.window_means(mrows, mtlen, geometric=True)
        sf = me.spec.get("scalefactor")
        if sf not in (None, 1):
            mu = torch.expm1(torch.log1p(mu) * sf)
        scale = torch.full((B,), 2.0 * ra, dtype=torch.float64, device=dev)
        return S, scale if delta is None or lowrank else scale * (1.0 - delta), scale * pdiag, -mu, None


class QEQW(Optimization):
    """P = 2 I, q = 0 (src/optimization.py:180-194)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.covariance = Covariance(method="duv")

    def set_objective(self, optimization_data: OptimizationData) -> None:
        X = optimization_data["return_series"]
        self.objective = Objective(P=self.covariance.estimate(X=X) * 2, q=np.zeros(X.shape[1]))

    def objective_batch(self, stage):
        import torch
        B, dev = stage.batch, stage.device
        return (stage.identity_P(), torch.full((B,), 2.0, dtype=torch.float64, device=dev),
                None, torch.zeros((B, stage.ld), dtype=torch.float64, device=dev), None)


def _tracking_rho_defaults(params) -> None:
    """ADMM start for tracking objectives (uncentred Gram P = 2 X'X, q = -2 X'y): rho =
    0.2 mean(diag P) and no |q| floor.  The floor (Settings.rho0_qrel) is for nearly linear
    mean-variance objectives; here |q| ~ diag P and it would start rho ~10x too high.
    Measured on the usa-shaped SPTR replication (494 assets, 4544 daily dates): 22 ADMM
    iterations and no refactorisation, against 168 iterations and 3744 refactorisations with
    the mean-variance defaults (7.6k -> 67.6k QPs/s, tools/diag_ls.py)."""
    params.setdefault("rho0_rel", 0.2)
    params.setdefault("rho0_qrel", 0.0)


class LeastSquares(Optimization):
    """P = 2 X'X (+ 2 l2 I), q = -2 X'y, constant y'y (src/optimization.py:198-229)."""

    def __init__(self, covariance: Optional[Covariance] = None, **kwargs):
        super().__init__(**kwargs)
        self.covariance = covariance
        _tracking_rho_defaults(self.params)

    def set_objective(self, optimization_data: OptimizationData) -> None:
        X = optimization_data["return_series"]
        y = optimization_data["bm_series"]
        if self.params.get("log_transform"):
            X = np.log(1 + X)
            y = np.log(1 + y)
        if isinstance(X, pd.DataFrame) and isinstance(y, (pd.DataFrame, pd.Series)):
            if not X.index.equals(y.index):
                # the reference's X.T @ y raises on misaligned dates (src/optimization.py:215-217)
                raise ValueError("matrices are not aligned")
        G, xty, yty = _device_gram(X, y)
        P = 2 * G
        l2 = self.params.get("l2_penalty")
        if l2 is not None and l2 != 0:
            P = P + 2 * l2 * np.eye(P.shape[0])
        if isinstance(X, pd.DataFrame):
            P = pd.DataFrame(P, index=X.columns, columns=X.columns)
        self.objective = Objective(P=P, q=-2 * xty, constant=yty)

    def objective_batch(self, stage):
        import torch
        if stage.panel.bm is None:
            return None
        from . import engine
        if self.params.get("log_transform"):
            pan = stage.log1p_panel()
        else:
            pan = stage.panel
        gp = stage.group_plan() if stage.prefer_lowrank else None
        if gp is not None and gp.ok:   # the window form with slide groups: X'y, y'y, diag(X'X) in one sliding pass
            dg = torch.zeros((stage.batch, stage.ld), dtype=torch.float64, device=stage.device)
            xty, yty = pan.gram_xy_grouped(gp, stage.tlen, dg=dg)
            G = None
            stage.lowrank = engine.LowRank(pan, stage.rows, stage.tlen, mu=None, dg=dg)
        else:
            if stage.prefer_lowrank:   # factored form X'X (uncentred) for the Woodbury solver (no n x n G)
                G = None
                stage.lowrank = engine.LowRank(pan, stage.rows, stage.tlen, mu=None)
            else:
                G = pan.cov(stage.rows, stage.tlen, mode=1, out=stage.P_buffer(), plan=stage.slide_plan())
            xty, yty = pan.gram_xy(stage.rows, stage.tlen)
        B, dev = stage.batch, stage.device
        l2 = self.params.get("l2_penalty")
        scale = torch.full((B,), 2.0, dtype=torch.float64, device=dev)
        pdiag = torch.full((B,), 2.0 * float(l2), dtype=torch.float64, device=dev) if l2 else None
        return G, scale, pdiag, -2.0 * xty, yty


class WeightedLeastSquares(Optimization):
    """P = 2 X'WX, q = -2 X'Wy with half-life tau weights (src/optimization.py:232-259)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        _tracking_rho_defaults(self.params)

    def _weights(self, T):
        lam = np.exp(-np.log(2) / self.params["tau"])
        w = lam ** np.arange(T)
        return np.flip(w / np.sum(w) * len(w))

    def set_objective(self, optimization_data: OptimizationData) -> None:
        X = optimization_data["return_series"]
        y = optimization_data["bm_series"]
        if self.params.get("log_transform"):
            X = np.log(1 + X)
            y = np.log(1 + y)
        Xv = np.asarray(to_numpy(X), dtype=np.float64)
        yv = np.asarray(to_numpy(y), dtype=np.float64).reshape(-1)
        sw = np.sqrt(self._weights(Xv.shape[0]))
        G, xty, yty = _device_gram(Xv * sw[:, None], yv * sw)
        self.objective = Objective(P=2 * G, q=-2 * xty, constant=yty)

    def objective_batch(self, stage):
        """Every date's WLS objective from one row-scaled panel.

        The reference's weights (src/optimization.py:242-246) are exponential in the row's
        age: the row r of the window ending at panel row e gets lam^(e - r) T / S_T, with
        S_T = sum_{i<T} lam^i.  Writing lam^(e - r) = lam^(a - r) lam^(e - a) for one anchor
        row a >= e of the whole chunk, the panel is scaled ONCE by sqrt(lam^(a - r)) and
        each date keeps a scalar c_e = lam^(e - a) T / S_T: X'WX = c_e Xs'Xs, X'Wy = c_e Xs'ys.
        K1 (Gram mode, sliding) or the window form then runs on the scaled panel unchanged,
        with c_e folded into p_scale (dense) or w_scale (window path)."""
        import torch
        from . import engine
        if stage.panel.bm is None:
            return None
        pan = stage.log1p_panel() if self.params.get("log_transform") else stage.panel
        lam = float(np.exp(-np.log(2) / self.params["tau"]))
        B, dev = stage.batch, stage.device
        t = stage.tlen_host.astype(np.int64)
        if np.any(t <= 0):
            return None
        # age counts window positions, not panel rows: rank every row the windows use
        # (weekend rows the builders drop are skipped) and require each window to be a run
        used = np.unique(np.concatenate([stage.rows_host[b, :t[b]] for b in range(B)]))
        pos = np.full(pan.D, -1, dtype=np.int64)
        pos[used] = np.arange(used.size)
        first = pos[stage.rows_host[:, 0]]
        last = pos[stage.rows_host[np.arange(B), t - 1]]
        if np.any(last - first != t - 1):
            return None
        a = int(last.max())
        if (a - int(first.min())) * -np.log2(lam) > 600:     # keep lam^(a - r) far from underflow
            return None
        age = np.where(pos >= 0, a - pos, 0)
        sw = torch.from_numpy(np.sqrt(lam ** age.astype(np.float64))).to(dev)
        span = engine.Panel(pan.R * sw[:, None], pan.bm * sw, device=dev)
        s_T = (1.0 - lam ** t) / (1.0 - lam) if lam < 1.0 else t.astype(np.float64)
        c = torch.from_numpy(lam ** (last - a).astype(np.float64) * t / s_T).to(dev)
        if stage.prefer_lowrank:
            G = None
            stage.lowrank = engine.LowRank(span, stage.rows, stage.tlen, mu=None, w_scale=c)
            scale = torch.full((B,), 2.0, dtype=torch.float64, device=dev)
        else:
            G = span.cov(stage.rows, stage.tlen, mode=1, out=stage.P_buffer(), plan=stage.slide_plan())
            scale = 2.0 * c
        xty, yty = span.gram_xy(stage.rows, stage.tlen)
        return G, scale, None, -2.0 * c[:, None] * xty, c * yty


class LAD(Optimization):
    """Least absolute deviation tracking (src/optimization.py:263-345): min sum |y - X w| as
    the reference's LP over [w; u; v].  solver_name 'mi355x' solves it with the batched
    device IPM of porqua_amd/lad.py; other names build the reference's dense LP for
    qpsolvers exactly as src/optimization.py:296-345 does."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.params["use_level"] = self.params.get("use_level", True)
        self.params["use_log"] = self.params.get("use_log", True)

    def set_objective(self, optimization_data: OptimizationData) -> None:
        X = optimization_data["return_series"]
        y = optimization_data["bm_series"]
        if self.params.get("use_level"):
            X = (1 + X).cumprod()
            y = (1 + y).cumprod()
            if self.params.get("use_log"):
                X = np.log(X)
                y = np.log(y)
        self.objective = Objective(X=X, y=y)

    def _bounds(self):
        boxed = self.constraints.box["box_type"] != "NA"
        lb = self.constraints.box["lower"].to_numpy(dtype=np.float64) if boxed else None
        ub = self.constraints.box["upper"].to_numpy(dtype=np.float64) if boxed else None
        return lb, ub

    def solve(self) -> bool:
        """src/optimization.py:286-294 (results hold the weights only, as there)."""
        universe = self.constraints.selection
        if self.params.get("solver_name") not in qp_problems.ENGINE_SOLVERS:
            self.model_qpsolvers()
            self.model.solve()
            x = self.model["solution"].x
        else:
            import torch
            from . import engine
            from . import lad as _lad
            if "leverage" in self.constraints.l1:
                raise TypeError("LAD with a leverage constraint: the reference's np.zeros() call "
                                "raises here (src/optimization.py:333)")
            X = np.ascontiguousarray(to_numpy(self.objective["X"]), dtype=np.float64)
            y = np.ascontiguousarray(to_numpy(self.objective["y"]), dtype=np.float64).reshape(-1)
            dev = engine.default_device()
            GhAb = self.constraints.to_GhAb()
            lb, ub = self._bounds()
            pr = _lad.LADProblem(torch.from_numpy(X)[None].to(dev), torch.from_numpy(y)[None].to(dev),
                                 A=GhAb["A"], b=GhAb["b"], G=GhAb["G"], h=GhAb["h"], lb=lb, ub=ub)
            res = _lad.lad_ipm_batched(pr)
            x = res.x[0].cpu().numpy() if bool(res.found[0]) else None
        w = x[:len(universe)] if x is not None else [None] * len(universe)
        self.results = {"weights": pd.Series(w, index=universe).to_dict()}
        return True

    def lad_batch(self, panel, rows, tlen, GhAb, lb, ub):
        """Every window of a backtest chunk in one device IPM: (W, status, obj) or None."""
        import torch
        from . import lad as _lad
        if panel.bm is None or len(tlen) == 0 or np.any(tlen != tlen[0]) or tlen[0] < 1:
            return None
        if "leverage" in self.constraints.l1:
            return None
        # the row table is padded to the longest window of the whole backtest: slice it to
        # this chunk's (uniform) window length, or the padding rows would join the LP
        rows = np.asarray(rows)[:, :int(tlen[0])]
        idx = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(panel.device)
        X, y = panel.R[idx], panel.bm[idx]
        if self.params.get("use_level"):
            X, y = torch.cumprod(1 + X, 1), torch.cumprod(1 + y, 1)
            if self.params.get("use_log"):
                X, y = torch.log(X), torch.log(y)
        pr = _lad.LADProblem(X.contiguous(), y.contiguous(), A=GhAb["A"], b=GhAb["b"], G=GhAb["G"],
                             h=GhAb["h"], lb=lb, ub=ub)
        res = _lad.lad_ipm_batched(pr)
        n = panel.n
        return res.x[:, :n].cpu().numpy(), res.status.cpu().numpy(), res.obj.cpu().numpy()

    def model_qpsolvers(self) -> None:
        """The reference's dense LP for a non-engine solver (src/optimization.py:296-345)."""
        X = to_numpy(self.objective["X"])
        y = to_numpy(self.objective["y"]).reshape(-1)
        GhAb = self.constraints.to_GhAb()
        N, T = X.shape[1], X.shape[0]
        G_t = np.pad(GhAb["G"], [(0, 0), (0, 2 * T)]) if GhAb["G"] is not None else None
        A = GhAb["A"]
        meq = 0 if A is None else 1 if A.ndim == 1 else A.shape[0]
        A_t = np.zeros((T, N + 2 * T)) if A is None else np.pad(np.atleast_2d(A), [(0, T), (0, 2 * T)])
        A_t[meq:T + meq, :N] = X
        A_t[meq:T + meq, N:N + T] = np.eye(T)
        A_t[meq:T + meq, N + T:] = -np.eye(T)
        b_t = y if GhAb["b"] is None else np.append(GhAb["b"], y)
        lb, ub = self._bounds()
        lb = np.pad(np.full(N, -np.inf) if lb is None else lb, (0, 2 * T))
        ub = np.pad(np.full(N, np.inf) if ub is None else ub, (0, 2 * T), constant_values=np.inf)
        if "leverage" in self.constraints.l1:
            raise TypeError("LAD with a leverage constraint: the reference's np.zeros() call raises "
                            "(src/optimization.py:333)")
        self.model = qp_problems.QuadraticProgram(P=np.zeros((N + 2 * T, N + 2 * T)),
                                                  q=np.append(np.zeros(N), np.ones(2 * T)),
                                                  G=G_t, h=GhAb["h"], A=A_t, b=b_t, lb=lb, ub=ub,
                                                  params=self.params)


class PercentilePortfolios(Optimization):
    """Quantile portfolios by score rank (src/optimization.py:356-417): the assets are cut
    into ``n_percentiles`` buckets at np.percentile thresholds of the negated scores;
    ``results['w_dict'][i]`` holds bucket i equally weighted, ``results['weights']`` the
    long-short portfolio bucket 1 minus bucket N.  The ranking runs on the device
    (engine.percentile_weights); ``percentile_batch`` ranks every date of a backtest at once.

    As in the reference, ``params`` becomes a plain dict {'solver_name', 'n_percentiles',
    'field'} (so any other keyword, the walkthrough's misspelt ``n_percentile`` included, is
    ignored), and the constraints the builders add are not used.  The reference's unseeded
    noise on exact-zero scores (src/optimization.py:393) is not reproduced: zeros tie like
    any equal scores."""

    def __init__(self, field: Optional[str] = None, estimator: Optional[MeanEstimator] = None,
                 n_percentiles=5, **kwargs):
        super().__init__(**kwargs)
        self.estimator = estimator
        self.params = {"solver_name": "percentile", "n_percentiles": n_percentiles, "field": field}

    def set_objective(self, optimization_data: OptimizationData) -> None:
        field = self.params.get("field")
        if self.estimator is not None:
            if field is not None:
                raise ValueError('Either specify a "field" or pass an "estimator", but not both.')
            scores = self.estimator.estimate(X=optimization_data["return_series"])
        elif field is not None:
            scores = optimization_data["scores"][field]
        else:
            score_weights = self.params.get("score_weights")
            if score_weights is not None:
                scores = (optimization_data["scores"][score_weights.keys()]
                          .multiply(score_weights.values()).sum(axis=1))
            else:
                scores = optimization_data["scores"].mean(axis=1).squeeze()
        self.objective = Objective(scores=-scores)

    def solve(self) -> bool:
        """src/optimization.py:398-417 on the device at batch 1.  An empty bucket (or a NaN
        score, which empties every bucket there) is the reference's ZeroDivisionError."""
        import torch
        from . import _lib, engine
        scores = self.objective["scores"]
        N = self.params["n_percentiles"]
        index = scores.index if hasattr(scores, "index") else pd.RangeIndex(len(scores))
        x = np.ascontiguousarray(to_numpy(scores), dtype=np.float64).reshape(1, -1)
        # the objective already holds -scores: the kernel ranks it as it is (sign +1)
        w, bucket, counts, _th, status = engine.percentile_weights(
            torch.from_numpy(x).to(engine.default_device()), N, sign=1.0)
        if int(status[0].item()) != _lib.PQ_PCT_OK:
            raise ZeroDivisionError("division by zero")
        self.results = percentile_results(index, w[0].cpu().numpy(), bucket[0].cpu().numpy(),
                                          counts[0].cpu().numpy())
        return True

    def percentile_batch(self, stage):
        """Every date of a backtest chunk in one launch: the device geometric means over each
        date's own estimator sub-window (MeanEstimator.window of that date's window length, so
        ragged early windows batch too), then engine.percentile_weights on the raw scores
        (sign -1).  Returns (w, bucket, counts, th, status) on the device, or None when the
        run has to take the serial loop (the ``field`` / ``scores`` forms, another estimator,
        a window the estimator leaves empty)."""
        import torch
        from . import engine
        me = self.estimator
        if me is None or self.params.get("field") is not None or me.spec.get("method") != "geometric":
            return None
        t = stage.tlen_host.astype(np.int64)
        if len(t) == 0:
            return None
        win = {int(v): me.window(int(v)) for v in np.unique(t)}
        a = np.array([win[int(v)][0] for v in t], dtype=np.int64)
        L = np.array([win[int(v)][1] for v in t], dtype=np.int64) - a
        if L.min() < 1:
            return None
        if not a.any() and np.array_equal(L, t):      # the whole window of every date
            gp = stage.group_plan()
            if gp.ok:   # slide groups: one sliding log-sum pass per group
                mu = stage.panel.window_geomeans_grouped(gp, stage.tlen)
            else:
                mu = stage.panel.window_means(stage.rows, stage.tlen, geometric=True)
        else:
            j = np.arange(int(L.max()), dtype=np.int64)[None, :]
            pos = np.minimum(a[:, None] + j, stage.rows_host.shape[1] - 1)
            mrows = np.take_along_axis(stage.rows_host, pos, axis=1) * (j < L[:, None])
            mrows, mtlen = stage.panel.rows_to_device(mrows, L)
            mu = stage.panel.window_means(mrows, mtlen, geometric=True)
        sf = me.spec.get("scalefactor")
        if sf not in (None, 1):
            mu = torch.expm1(torch.log1p(mu) * sf)
        return engine.percentile_weights(mu, self.params["n_percentiles"], sign=-1.0, n=stage.n)


def percentile_results(index, w, bucket, counts) -> dict:
    """``PercentilePortfolios.results`` of one date with the reference's types
    (src/optimization.py:411-416): 'weights' a dict over the universe, 'w_dict' {i: Series over
    bucket i's members in universe order, each 1 / len(bucket i)}."""
    index = index if isinstance(index, pd.Index) else pd.Index(index)
    w_dict = {}
    for i in range(1, len(counts) + 1):
        members = np.flatnonzero(bucket == i)
        w_dict[i] = pd.Series(np.full(len(members), 1 / int(counts[i - 1])), index=index[members])
    return {"weights": dict(zip(index, w.tolist())), "w_dict": w_dict}


def covariance_window_form(covariance, panel, rows, tlen, dg):
    """(a, c) per date (device tensors) of the window form Sigma = a Xc'Xc + c I of a Covariance
    spec -- 'pearson' (1/(T-1), 0), 'linear_shrinkage' c = lambda mean(diag S), 'ledoit_wolf' /
    'oas' ((1-delta)/(T-1), delta mean(diag S)) with the intensity of engine.shrinkage_intensity
    (left in ``covariance.shrinkage_batch_``), 'duv' (0, 1) --, shared by RiskParity and
    HierarchicalRiskParity.  ``dg``: diag(Xc'Xc) of every window (Panel.window_sumsq)."""
    import torch
    from . import engine
    from .covariance import SHRINKAGE_METHODS, _shrink_lambda
    method = covariance.spec["method"]
    B, dev = int(rows.shape[0]), panel.device
    if method == "duv":
        return (torch.zeros(B, dtype=torch.float64, device=dev),
                torch.ones(B, dtype=torch.float64, device=dev))
    a = 1.0 / (tlen.to(torch.float64) - 1.0)
    md = dg[:, :panel.n].mean(dim=1) * a          # mean(diag S)
    if method == "pearson":
        return a, torch.zeros_like(a)
    if method == "linear_shrinkage":
        return a, _shrink_lambda(covariance.spec.get("lambda_covmat_regularization")) * md
    if method in SHRINKAGE_METHODS:
        delta, _ = engine.shrinkage_intensity(panel, rows, tlen, kind=method)
        covariance.shrinkage_batch_ = delta
        return (1.0 - delta) * a, delta * md
    if method == "ewma":
        raise NotImplementedError("the 'ewma' covariance has no window form Sigma = a Xc'Xc + c I: its rows carry "
                                  "one weight each, which a scalar a per date cannot express")
    raise NotImplementedError("This method is not implemented yet")


RP_NAN_MESSAGE = "RiskParity: missing values in the return window are not supported"
RP_REASONS = {1: "no convergence within max_sweeps sweeps",
              2: "bad input (a zero-variance asset without a ridge, a one-row window, or non-finite data)"}


class RiskParity(Optimization):
    """Risk-parity / risk-budgeting portfolios (equal risk contribution by default): the weights
    x > 0 with sum x = budget at which asset i carries the share b_i of the portfolio variance,
    x_i (Sigma x)_i / x' Sigma x = b_i.  Not a QP: Spinu's convex form
    y* = argmin_{y > 0} 1/2 y' Sigma y - sum_i b_i log y_i, x = budget y* / sum(y*), solved by
    cyclical coordinate descent on the device (engine.risk_parity_weights, pq_risk_parity_batched)
    on the window form Sigma = a Xc'Xc + c I of the ``covariance`` spec: 'pearson' (1/(T-1), 0),
    'linear_shrinkage' c = lambda mean(diag S), 'ledoit_wolf' / 'oas' ((1-delta)/(T-1),
    delta mean(diag S)) with the intensity of engine.shrinkage_intensity, 'duv' (0, 1).  'pca':
    the uncentred form (1, sigma2) of the k factor rows of engine.pca_window_form, built once per
    ``solve_windows``; the per-date factor counts and noise levels stay in the covariance's
    ``n_factors_batch_`` / ``noise_variance_batch_``, and a date whose factor model is bad input
    (sigma2 NaN) is PQ_RP_BAD_INPUT.  'gerber' is not served (NotImplementedError): the kernel
    needs a window form, and the Gerber thresholds are per date, so no rows are shared; nor are
    'spearman' and 'kendall' (NotImplementedError): the ranks belong to each date's own window;
    nor is 'ewma' (NotImplementedError): its rows carry one weight each, and the kernel's window
    form has a single scalar a per date.

    ``risk_budget``: a dict or Series over the assets (None: equal budgets); an asset of the
    date's selection without an entry is an error, entries must be > 0, and the budgets are
    normalised to sum 1 over the selection.  ``params``: ``eps`` (1e-10, the relative residual
    max_i |y_i (Sigma y)_i - b_i| / b_i at which a date is solved) and ``max_sweeps`` (500).

    * Of the constraints only the budget's right-hand side is used, as the sum of the weights
      (1 without a budget constraint).  Box and linear constraints are ignored -- the portfolio
      is long-only by construction --, as PercentilePortfolios ignores the builders' constraints.
    * ``check_positive_definite`` is moot: the window form is positive semi-definite.
    * Missing values in the return window are not supported: ``solve()`` raises ValueError, a
      backtest RuntimeError, with RP_NAN_MESSAGE.

    ``solve()`` runs the kernel at batch 1 and fills ``results`` = {'weights', 'status',
    'risk_contributions'}; ``status`` is False unless the date is PQ_RP_OK (the weights are then
    None).  ``risk_parity_batch`` solves every date of a backtest chunk in one launch."""

    def __init__(self, covariance: Optional[Covariance] = None, risk_budget=None, **kwargs):
        super().__init__(**kwargs)
        self.covariance = Covariance() if covariance is None else covariance
        self.risk_budget = risk_budget
        self.params.setdefault("eps", 1e-10)
        self.params.setdefault("max_sweeps", 500)

    def set_objective(self, optimization_data: OptimizationData) -> None:
        self.objective = Objective(X=optimization_data["return_series"])

    def budget_vector(self, universe) -> np.ndarray:
        """The risk budgets over ``universe``, normalised to sum 1."""
        universe = list(universe)
        if self.risk_budget is None:
            return np.full(len(universe), 1.0 / len(universe))
        rb = self.risk_budget if isinstance(self.risk_budget, pd.Series) else pd.Series(dict(self.risk_budget))
        missing = [a for a in universe if a not in rb.index]
        if missing:
            raise ValueError(f"RiskParity: risk_budget has no entry for {missing[:5]}"
                             + (" ..." if len(missing) > 5 else ""))
        b = rb.reindex(universe).to_numpy(dtype=np.float64)
        if not np.all(np.isfinite(b)) or not np.all(b > 0):
            raise ValueError("RiskParity: risk budgets must be finite and > 0")
        return b / b.sum()

    def budget_scale(self) -> float:
        rhs = self.constraints.budget.get("rhs")
        return 1.0 if rhs is None else float(rhs)

    def window_form(self, panel, rows, tlen, dg):
        """(a, c) per date of Sigma = a Xc'Xc + c I for the covariance spec (device tensors)."""
        return covariance_window_form(self.covariance, panel, rows, tlen, dg)

    def solve_windows(self, panel, rows, tlen, universe):
        """Every window of the device row table in one launch -> (x, stats, status, form) on the
        device; form = (mu, a, c), what risk_contributions needs, or (None, a, c, pca form) with
        the 'pca' covariance: the window is then the date's factor rows."""
        from . import engine
        if panel.has_nan:
            raise ValueError(RP_NAN_MESSAGE)
        if self.covariance.spec["method"] == "pca":
            pf = self.covariance.window_form_pca(panel, rows, tlen)
            a = pf.sigma2.new_ones(pf.sigma2.shape)
            x, stats, status = engine.risk_parity_weights(
                pf.panel, pf.rows, pf.tlen, budgets=self.budget_vector(universe), a=a, c=pf.sigma2, centred=False,
                scale=self.budget_scale(), eps=float(self.params["eps"]), max_sweeps=int(self.params["max_sweeps"]))
            return x, stats, status, (None, a, pf.sigma2, pf)
        mu = panel.window_means(rows, tlen)
        dg = panel.window_sumsq(rows, tlen, mu)
        a, c = self.window_form(panel, rows, tlen, dg)
        x, stats, status = engine.risk_parity_weights(
            panel, rows, tlen, budgets=self.budget_vector(universe), a=a, c=c, scale=self.budget_scale(),
            eps=float(self.params["eps"]), max_sweeps=int(self.params["max_sweeps"]), moments=(mu, dg))
        return x, stats, status, (mu, a, c)

    @staticmethod
    def risk_contributions(panel, rows, tlen, form, x, i: int) -> np.ndarray:
        """x_j (Sigma x)_j / x' Sigma x of date i from the window form (torch, on the device)."""
        mu, a, c = form[:3]
        if len(form) > 3:   # the 'pca' covariance: the uncentred factor rows of the date
            panel, rows, tlen = form[3].panel, form[3].rows, form[3].tlen
        T = int(tlen[i].item())
        X = panel.R[rows[i, :T].long()]
        if mu is not None:
            X = X - mu[i, :panel.n]
        xi = x[i]
        m = xi * (a[i] * (X.T @ (X @ xi)) + c[i] * xi)
        return (m / m.sum()).cpu().numpy()

    def solve(self) -> bool:
        from . import _lib, engine
        X = self.objective["X"]
        universe = list(X.columns) if isinstance(X, pd.DataFrame) else list(self.constraints.selection)
        Xv = np.ascontiguousarray(to_numpy(X), dtype=np.float64)
        if np.isnan(Xv).any():
            raise ValueError(RP_NAN_MESSAGE)
        T = Xv.shape[0]
        panel = engine.Panel(Xv)
        rows, tlen = panel.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
        x, stats, status, form = self.solve_windows(panel, rows, tlen, universe)
        ok = int(status[0].item()) == _lib.PQ_RP_OK
        w = x[0].cpu().numpy().tolist() if ok else [None] * len(universe)
        rc = self.risk_contributions(panel, rows, tlen, form, x, 0).tolist() if ok else [None] * len(universe)
        self.results = {"weights": dict(zip(universe, w)), "status": ok,
                        "risk_contributions": dict(zip(universe, rc))}
        return ok

    def risk_parity_batch(self, stage):
        """Every date of a backtest chunk in one launch (the counterpart of
        PercentilePortfolios.percentile_batch): (x, stats, status, form) on the device, the
        assets being the constraints' selection (date-invariant builders)."""
        if stage.batch == 0:
            return None
        return self.solve_windows(stage.panel, stage.rows, stage.tlen, self.constraints.selection)


HRP_NAN_MESSAGE = "HierarchicalRiskParity: missing values in the return window are not supported"
HRP_REASON = "bad input (a zero-variance asset without a ridge, a one-row window, or non-finite data)"
HRP_LINKAGES = ("single", "complete", "average", "weighted")


class HierarchicalRiskParity(Optimization):
    """Hierarchical risk parity (Lopez de Prado 2016): the tree of the correlation distance
    sqrt((1 - rho) / 2) as SciPy's linkage builds it, the assets in its leaf order, and the
    recursive bisection of that order, each half weighted by the other's inverse-variance cluster
    variance.  Not a QP and nothing is inverted or factored, so it is defined where the sample
    covariance is singular (more assets than window rows).  Every date is one workgroup of
    pq_hrp_batched (engine.hrp_weights) on the dense Sigma of the ``covariance`` spec: 'pearson',
    'linear_shrinkage', 'ledoit_wolf' / 'oas' (the intensity of engine.shrinkage_intensity), 'duv'
    -- the (a, c) mapping of RiskParity (covariance_window_form), as Sigma = alpha S + c I on the
    sample covariance S; 'pca': S the Gram Z'Z of the k factor rows of engine.pca_window_form with
    alpha = 1 and c = sigma2 (a date whose factor model is bad input is PQ_HRP_BAD_INPUT); 'gerber':
    S the dense estimate of engine.gerber_cov per chunk of dates, alpha = 1 and c = 0 (a bad-input
    date arrives as NaN and is PQ_HRP_BAD_INPUT by the kernel's own check); 'spearman' / 'kendall':
    the dense estimate of engine.rank_cov in the same way; 'ewma': the dense estimate of
    engine.ewma_cov (its direct kernel) in the same way.
    ``linkage``: 'single' (Lopez de Prado's choice, the default), 'complete',
    'average' or 'weighted', with SciPy's meaning; any other name raises NotImplementedError --
    'ward' too, though the kernel has it: engine.hrp_weights(method='ward') reaches it --, and
    'centroid' and 'median' are not built at all (their trees can invert).  At most
    _lib.PQ_HRP_NMAX assets.

    * Of the constraints only the budget's right-hand side is used, as the sum of the weights
      (1 without a budget constraint).  Box and linear constraints are ignored -- the portfolio
      is long-only by construction --, as RiskParity ignores them.
    * Missing values in the return window are not supported: ``solve()`` raises ValueError, a
      backtest RuntimeError, with HRP_NAN_MESSAGE.

    ``solve()`` runs the kernel at batch 1 and fills ``results`` = {'weights', 'status', 'order'
    (the asset names in leaf order), 'linkage' (SciPy's Z as a numpy array)}; ``status`` is False
    unless the date is PQ_HRP_OK (the weights are then None).  ``hrp_batch`` solves every date of
    a backtest chunk."""

    def __init__(self, covariance: Optional[Covariance] = None, linkage: str = "single", **kwargs):
        super().__init__(**kwargs)
        if linkage not in HRP_LINKAGES:
            raise NotImplementedError(f"HierarchicalRiskParity: linkage '{linkage}' is not implemented (only "
                                      + ", ".join(f"'{name}'" for name in HRP_LINKAGES) + ")")
        self.covariance = Covariance() if covariance is None else covariance
        self.linkage = linkage

    def set_objective(self, optimization_data: OptimizationData) -> None:
        self.objective = Objective(X=optimization_data["return_series"])

    def budget_scale(self) -> float:
        rhs = self.constraints.budget.get("rhs")
        return 1.0 if rhs is None else float(rhs)

    def solve_windows(self, panel, rows, tlen, linkage: bool = False):
        """Every window of the device row table -> engine.hrp_weights' tuple, on the device."""
        from . import engine
        if panel.has_nan:
            raise ValueError(HRP_NAN_MESSAGE)
        if self.covariance.spec["method"] == "pca":   # Sigma = Z'Z + sigma2 I on the factor rows Z
            pf = self.covariance.window_form_pca(panel, rows, tlen)
            return engine.hrp_weights(pf.panel, pf.rows, pf.tlen, alpha=1.0, c=pf.sigma2, centred=False,
                                      scale=self.budget_scale(), linkage=linkage, method=self.linkage)
        if self.covariance.spec["method"] == "gerber":   # the dense Gerber estimate in place of Panel.cov
            threshold, variant = self.covariance.gerber_spec

            def dense(r, t, out):
                return engine.gerber_cov(panel, r, t, threshold=threshold, variant=variant, out=out)[0]
            return engine.hrp_weights(panel, rows, tlen, alpha=1.0, c=0.0, scale=self.budget_scale(),
                                      linkage=linkage, method=self.linkage, dense=dense)
        if self.covariance.spec["method"] in RANK_METHODS:   # the dense rank estimate in place of Panel.cov
            kind = self.covariance.spec["method"]

            def dense(r, t, out):
                return engine.rank_cov(panel, r, t, kind=kind, out=out)[0]
            return engine.hrp_weights(panel, rows, tlen, alpha=1.0, c=0.0, scale=self.budget_scale(),
                                      linkage=linkage, method=self.linkage, dense=dense)
        if self.covariance.spec["method"] == "ewma":   # the dense exponentially weighted estimate
            halflife, decay = self.covariance.ewma_spec

            def dense(r, t, out):
                return engine.ewma_cov(panel, r, t, halflife=halflife, decay=decay, out=out)[0]
            return engine.hrp_weights(panel, rows, tlen, alpha=1.0, c=0.0, scale=self.budget_scale(),
                                      linkage=linkage, method=self.linkage, dense=dense)
        mu = panel.window_means(rows, tlen)
        dg = panel.window_sumsq(rows, tlen, mu)
        a, c = covariance_window_form(self.covariance, panel, rows, tlen, dg)
        # Sigma = a Xc'Xc + c I = alpha S + c I on the sample covariance S = Xc'Xc / (T - 1)
        alpha = a * (tlen.to(a.dtype) - 1.0)
        return engine.hrp_weights(panel, rows, tlen, alpha=alpha, c=c, scale=self.budget_scale(), linkage=linkage,
                                  method=self.linkage)

    def solve(self) -> bool:
        from . import _lib, engine
        X = self.objective["X"]
        universe = list(X.columns) if isinstance(X, pd.DataFrame) else list(self.constraints.selection)
        Xv = np.ascontiguousarray(to_numpy(X), dtype=np.float64)
        if np.isnan(Xv).any():
            raise ValueError(HRP_NAN_MESSAGE)
        T = Xv.shape[0]
        panel = engine.Panel(Xv)
        rows, tlen = panel.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
        x, order, stats, status, Z = self.solve_windows(panel, rows, tlen, linkage=True)
        ok = int(status[0].item()) == _lib.PQ_HRP_OK
        w = x[0].cpu().numpy().tolist() if ok else [None] * len(universe)
        leaf = [universe[i] for i in order[0].cpu().numpy().tolist()] if ok else None
        self.results = {"weights": dict(zip(universe, w)), "status": ok, "order": leaf,
                        "linkage": Z[0].cpu().numpy() if ok else None}
        return ok

    def hrp_batch(self, stage):
        """Every date of a backtest chunk (the counterpart of RiskParity.risk_parity_batch):
        (x, order, stats, status, Z) on the device, the assets being the constraints' selection
        (date-invariant builders)."""
        if stage.batch == 0:
            return None
        return self.solve_windows(stage.panel, stage.rows, stage.tlen, linkage=True)
