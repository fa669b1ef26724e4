"""Extended-precision model of the risk-parity (risk-budgeting) solve, independent of the engine.

Spinu's convex form  y* = argmin_{y > 0} 1/2 y' Sigma y - sum_i b_i log y_i,  x = scale y* / sum y*,
by cyclical coordinate descent (Griveau-Billion, Richard, Roncalli 2013) on the DENSE Sigma in
np.longdouble, one coordinate at a time in the order 0..n-1 from y_i = sqrt(b_i / Sigma_ii):

    s_i = (Sigma y)_i - Sigma_ii y_i,    y_i <- (-s_i + sqrt(s_i^2 + 4 Sigma_ii b_i)) / (2 Sigma_ii)

Nothing here is blocked, tiled or kept in window form: the kernel's 16-asset blocked recurrence
is the same ordered recurrence in exact arithmetic, so its k-th iterate has to match
``iterate(S, b, k)`` up to rounding.  ``blocked_f64`` is the float64 numpy restatement of the
blocked window form (no Sigma, r = Xc y carried along); the tests measure its distance from the
model to size their tolerances.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble


def window(R, rows, centred=True):
    """The date's T x n window of the panel in longdouble, centred by its own column means."""
    X = np.asarray(R, dtype=np.float64)[np.asarray(rows, dtype=np.int64)].astype(LD)
    return X - X.mean(axis=0) if centred else X


def sigma(X, a, c):
    """Sigma = a X'X + c I (dense, longdouble) of a (centred) window X."""
    X = np.asarray(X, dtype=LD)
    n = X.shape[1]
    return LD(a) * (X.T @ X) + LD(c) * np.eye(n, dtype=LD)


def start(S, b):
    return np.sqrt(np.asarray(b, dtype=LD) / np.diag(S))


def sweep(S, b, y):
    """One ordered pass over the coordinates, in place."""
    n = len(y)
    for i in range(n):
        d = S[i, i]
        s = S[i] @ y - d * y[i]
        y[i] = (-s + np.sqrt(s * s + 4 * d * b[i])) / (2 * d)
    return y


def iterate(S, b, k):
    """The k-th iterate (k = 0: the start)."""
    S = np.asarray(S, dtype=LD)
    b = np.asarray(b, dtype=LD)
    y = start(S, b)
    for _ in range(int(k)):
        sweep(S, b, y)
    return y


def residual(S, b, y):
    """max_i |y_i (Sigma y)_i - b_i| / b_i."""
    S = np.asarray(S, dtype=LD)
    b = np.asarray(b, dtype=LD)
    y = np.asarray(y, dtype=LD)
    return float(np.max(np.abs(y * (S @ y) - b) / b))


def objective(S, b, y):
    y = np.asarray(y, dtype=LD)
    return LD(0.5) * (y @ (S @ y)) - np.asarray(b, dtype=LD) @ np.log(y)


def solve(S, b, eps=1e-14, max_sweeps=5000):
    """(y, sweeps, res): sweeps until the relative residual is <= eps (or max_sweeps)."""
    S = np.asarray(S, dtype=LD)
    b = np.asarray(b, dtype=LD)
    y = start(S, b)
    k, res = 0, residual(S, b, y)
    while res > eps and k < max_sweeps:
        sweep(S, b, y)
        k += 1
        res = residual(S, b, y)
    return y, k, res


def weights(y, scale=1.0):
    y = np.asarray(y, dtype=LD)
    return LD(scale) * y / y.sum()


def risk_contributions(S, x):
    """x_i (Sigma x)_i / x' Sigma x."""
    S = np.asarray(S, dtype=LD)
    x = np.asarray(x, dtype=LD)
    m = x * (S @ x)
    return m / m.sum()


def record(S, b, x, sum_y):
    """(res, x' Sigma x, sum y) of a returned pair (x, sum y) with sum x = scale: the y behind it
    is x sum_y / scale."""
    x = np.asarray(x, dtype=LD)
    scale = x.sum()
    y = x * (LD(sum_y) / scale)
    return residual(S, b, y), float(x @ (np.asarray(S, dtype=LD) @ x)), float(y.sum())


def equal_budget(n):
    return np.full(n, 1.0 / n)


def skewed_budget(n):
    """Linearly skewed budgets: b_i proportional to 1 + i (sum 1)."""
    w = 1.0 + np.arange(n, dtype=np.float64)
    return w / w.sum()


def blocked_f64(Xc, a, c, b, eps=1e-10, max_sweeps=500, tile=16):
    """Float64 restatement of the blocked window form: r = Xc y carried along, 16 assets per
    step (G = a Xt'Xt, g = a Xt'r, the serial chain, then r += Xt delta).  The residual after
    every sweep is evaluated with r recomputed from y.  Returns (y, sweeps, res)."""
    Xc = np.ascontiguousarray(Xc, dtype=np.float64)
    T, n = Xc.shape
    b = np.asarray(b, dtype=np.float64)
    dg = np.einsum("ti,ti->i", Xc, Xc)
    d = a * dg + c
    y = np.sqrt(b / d)
    r = Xc @ y

    def res_of(y):
        rr = Xc @ y
        return float(np.max(np.abs(y * (a * (Xc.T @ rr) + c * y) - b) / b))

    k, res = 0, res_of(y)
    while k < max_sweeps and not res <= eps:
        for j0 in range(0, n, tile):
            Xt = Xc[:, j0:j0 + tile]
            m = Xt.shape[1]
            G = a * (Xt.T @ Xt)
            g = a * (Xt.T @ r)
            delta = np.zeros(m)
            for i in range(m):
                j = j0 + i
                s = g[i] + G[i, :i] @ delta[:i] - a * dg[j] * y[j]
                q = np.sqrt(s * s + 4.0 * d[j] * b[j])
                ynew = 2.0 * b[j] / (s + q) if s > 0 else (q - s) / (2.0 * d[j])
                delta[i] = ynew - y[j]
                y[j] = ynew
            r += Xt @ delta
        k += 1
        res = res_of(y)
    return y, k, res
