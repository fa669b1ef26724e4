"""Independent model of the engine's result record (test helper; host only, np.longdouble).

Every answer of the engine carries out[PQ_OUT_OBJ | PRIM | DUAL | GAP], written on the device by
the polish kernel that scored the point (polish.hip, polish_w.hip, polish_g.hip) or on the host
from a device P x (qp_problems._solve_batch_ipm).  This module recomputes those four numbers
from the problem data and the returned point (x, y, z_box) alone, in extended precision, with the
qpsolvers definitions of oracle/qp_ipm.py:50-90 and qp_problems._residuals:

    obj  = 1/2 x'Px + q'x
    prim = max(|Cx - b| on equality rows, [Cx - ug]+, [lg - Cx]+, [lb - x]+, [x - ub]+, 0)
    dual = || Px + q + C'y + z_box ||inf
    gap  = | x'Px + q'x + sum_r bound_r y_r + lb'min(z_box, 0) + ub'max(z_box, 0) |
           bound_r = ug_r if y_r > 0 else lg_r; infinite bounds contribute 0

for the two forms of P the engine knows:

    dense   P_eff = p_scale P + p_diag I
    window  P_eff = p_scale w_scale (X - 1 mu')'(X - 1 mu') + p_diag I     (mu None: uncentred)

General rows are in the engine's storage lg <= C x <= ug (equalities have lg == ug); infinite
sides are allowed in lg, ug, lb, ub and the box may be absent.

The comparison bar is derived, not measured.  With each quantity the model returns its
absolute-term sum S -- the same expression with every product replaced by its absolute value;
the window form uses A = |X| + |1 mu'| in place of |X - 1 mu'|, so the bound also holds for the
kernels' algebra u_t = X_t x - mu x (polish_dev.h) -- and

    |engine - model| <= N u S,   u = 2^-53,
    N = 2 (n + T + mg + 16)  (window form),   N = 2 (n + mg + 16)  (dense form):

the classical gamma_m sum|terms| bound of a length-m FP64 sum over the longest chain of sums
behind a field (C x or C'y, then X x, then X'u; the final dot with x for obj and gap is covered
by the doubling), doubled for the scalings and the centring.  For the two max-norms S is taken
per component and the bar is max_i N u S_i, since |max|a| - max|b|| <= max|a - b|.  The kernels'
tree and MFMA sums have shorter chains than the bound assumes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FIELDS = ("obj", "prim", "dual", "gap")


@dataclass
class Record:
    obj: float
    prim: float
    dual: float
    gap: float
    S: dict          # absolute-term sum of each field (prim / dual: the largest component's)
    N: int           # chain-length factor of the bar
    scale: float     # the kernels' problem scale max(||q||inf, max_i |P_eff,ii|)
    Px: np.ndarray   # P_eff x (longdouble)
    S_Px: np.ndarray

    def bar(self, field: str) -> float:
        return self.N * U * self.S[field]

    def value(self, field: str) -> float:
        return getattr(self, field)

    def units(self, field: str, engine_value: float) -> float:
        """|engine - model| in units of u S (the bar is N of these)."""
        d = abs(LD(engine_value) - LD(getattr(self, field)))
        s = self.S[field]
        return float(d / (U * s)) if s > 0 else (0.0 if d == 0 else np.inf)


def _ld(v, shape=None):
    a = np.asarray(v, dtype=LD)
    return a if shape is None else a.reshape(shape)


def _finite(v):
    """v with its infinite entries replaced by 0 (they contribute nothing)."""
    return np.where(np.isfinite(v), v, LD(0))


def _score(n, Px, S_Px, scale, N, q, x, y, z_box, C, lg, ug, lb, ub) -> Record:
    q, x = _ld(q, n), _ld(x, n)
    ax, aq = np.abs(x), np.abs(q)
    mg = 0 if C is None else np.asarray(C).reshape(-1, n).shape[0]
    zb = np.zeros(n, dtype=LD) if z_box is None else _ld(z_box, n)

    obj = LD(0.5) * (x @ Px) + q @ x
    S_obj = LD(0.5) * (ax @ S_Px) + aq @ ax
    g = Px + q + zb
    S_g = S_Px + aq + np.abs(zb)
    gap = x @ Px + q @ x
    S_gap = ax @ S_Px + aq @ ax

    viol = [LD(0)]        # components of the primal residual and their absolute-term sums
    S_viol = [LD(0)]
    if mg:
        C = _ld(C, (mg, n))
        lg, ug, y = _ld(lg, mg), _ld(ug, mg), _ld(y, mg)
        Cx, S_Cx = C @ x, np.abs(C) @ ax
        g = g + C.T @ y
        S_g = S_g + np.abs(C).T @ np.abs(y)
        for r in range(mg):
            if lg[r] == ug[r]:
                viol.append(abs(Cx[r] - ug[r]))
                S_viol.append(S_Cx[r] + abs(ug[r]))
            else:
                if np.isfinite(ug[r]):
                    viol.append(Cx[r] - ug[r])
                    S_viol.append(S_Cx[r] + abs(ug[r]))
                if np.isfinite(lg[r]):
                    viol.append(lg[r] - Cx[r])
                    S_viol.append(S_Cx[r] + abs(lg[r]))
        bound = _finite(np.where(y > 0, ug, lg))
        gap = gap + bound @ y
        S_gap = S_gap + np.abs(bound) @ np.abs(y)
    if lb is not None:
        lo = _ld(lb, n)
        fin = np.isfinite(lo)
        viol += list((lo - x)[fin])
        S_viol += list((np.abs(lo) + ax)[fin])
        gap = gap + _finite(lo) @ np.minimum(zb, 0)
        S_gap = S_gap + np.abs(_finite(lo)) @ np.abs(np.minimum(zb, 0))
    if ub is not None:
        up = _ld(ub, n)
        fin = np.isfinite(up)
        viol += list((x - up)[fin])
        S_viol += list((np.abs(up) + ax)[fin])
        gap = gap + _finite(up) @ np.maximum(zb, 0)
        S_gap = S_gap + np.abs(_finite(up)) @ np.maximum(zb, 0)
    S = {"obj": float(S_obj), "prim": float(max(S_viol)), "dual": float(S_g.max()), "gap": float(S_gap)}
    return Record(obj=float(obj), prim=float(max(viol)), dual=float(np.abs(g).max()), gap=float(abs(gap)),
                  S=S, N=int(N), scale=float(scale), Px=Px, S_Px=S_Px)


def dense_record(P, q, x, y=None, z_box=None, C=None, lg=None, ug=None, lb=None, ub=None,
                 p_scale=1.0, p_diag=0.0) -> Record:
    """The record of the point (x, y, z_box) for P_eff = p_scale P + p_diag I."""
    n = len(x)
    P, xl = _ld(P, (n, n)), _ld(x, n)
    ps, pd = LD(p_scale), LD(p_diag)
    Px = ps * (P @ xl) + pd * xl
    S_Px = abs(ps) * (np.abs(P) @ np.abs(xl)) + np.abs(pd * xl)
    scale = max(float(np.abs(_ld(q, n)).max(initial=0)), float(np.abs(ps * np.diag(P) + pd).max()))
    mg = 0 if C is None else np.asarray(C).reshape(-1, n).shape[0]
    return _score(n, Px, S_Px, scale, 2 * (n + mg + 16), q, x, y, z_box, C, lg, ug, lb, ub)


def window_record(X, mu, q, x, y=None, z_box=None, C=None, lg=None, ug=None, lb=None, ub=None,
                  p_scale=1.0, w_scale=1.0, p_diag=0.0) -> Record:
    """The record for P_eff = p_scale w_scale (X - 1 mu')'(X - 1 mu') + p_diag I: ``X`` the
    window's panel rows (T x n), ``mu`` the vector the engine was given (None: uncentred)."""
    n = len(x)
    X = _ld(X).reshape(-1, n)
    T = X.shape[0]
    xl = _ld(x, n)
    c, pd = LD(p_scale) * LD(w_scale), LD(p_diag)
    A = np.abs(X)
    Xc = X
    if mu is not None:
        m = _ld(mu, n)
        Xc = X - m[None, :]
        A = A + np.abs(m)[None, :]
    Px = c * (Xc.T @ (Xc @ xl)) + pd * xl
    S_Px = abs(c) * (A.T @ (A @ np.abs(xl))) + np.abs(pd * xl)
    scale = max(float(np.abs(_ld(q, n)).max(initial=0)), float(np.abs(c * (Xc * Xc).sum(0) + pd).max()))
    mg = 0 if C is None else np.asarray(C).reshape(-1, n).shape[0]
    return _score(n, Px, S_Px, scale, 2 * (n + T + mg + 16), q, x, y, z_box, C, lg, ug, lb, ub)


def rows_from_qp(A=None, b=None, G=None, h=None, n=None):
    """qpsolvers' A x = b, G x <= h in the engine's row storage: (C, lg, ug), equalities first."""
    Cs, lo, up = [], [], []
    if A is not None:
        A = np.asarray(A, dtype=np.float64).reshape(-1, n)
        b = np.asarray(b, dtype=np.float64).reshape(-1)
        Cs.append(A); lo.append(b); up.append(b)
    if G is not None:
        G = np.asarray(G, dtype=np.float64).reshape(-1, n)
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        Cs.append(G); lo.append(np.full(len(h), -np.inf)); up.append(h)
    if not Cs:
        return None, None, None
    return np.vstack(Cs), np.concatenate(lo), np.concatenate(up)


def duals_from_qp(y=None, z=None):
    """qpsolvers' (y, z) as the engine's multiplier vector of the general rows (y first)."""
    parts = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (y, z) if v is not None]
    return np.concatenate(parts) if parts else np.zeros(0)
