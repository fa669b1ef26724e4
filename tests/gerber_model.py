"""NumPy model of the Gerber covariance (Gerber, Markowitz, Ernst, Miao, Javid, Sargen 2022) as
include/porqua_hip.h defines it for pq_gerber_cov_batched.

For one T x n window X of raw returns (not demeaned) and a threshold 0 < c <= 1:
    m_k the window mean, dg_k = sum_t (x_tk - m_k)^2 (two passes), sd_k = sqrt(dg_k / (T - 1)),
    h_k = c sd_k, s_tk = +1 if x_tk >= h_k, -1 if x_tk <= -h_k, else 0,
    a_k = sum_t |s_tk|, H = S'S, P = |S|'|S| (integers),
    variant 2: g_ij = H_ij / sqrt(a_i a_j);   variant 1: g_ij = H_ij / (a_i + a_j - P_ij),
    Sigma_ij = g_ij (sd_i sd_j).
A window is bad input where T < 2, a value is not finite, some dg_k = 0 or some a_k = 0.
Everything is float64 and int64: the counts are exact, variant 1's g is one IEEE division of two
integers, variant 2's one square root of an exact product and one division."""
from collections import namedtuple

import numpy as np

OK, BAD_INPUT = 0, 1

Gerber = namedtuple("Gerber", "status sd h S a H P G Sigma")


def moments(X):
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    m = X.sum(axis=0) / T
    dg = ((X - m) ** 2).sum(axis=0)
    return m, dg


def signs(X, c):
    """(sd, h, S int64 [T, n]) of a window with T >= 2."""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    _, dg = moments(X)
    sd = np.sqrt(dg / (T - 1))
    h = c * sd
    S = (X >= h).astype(np.int64) - (X <= -h).astype(np.int64)
    return sd, h, S


def gerber(X, c=0.5, variant=2):
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    bad = Gerber(BAD_INPUT, None, None, None, None, None, None, np.full((n, n), np.nan), np.full((n, n), np.nan))
    if T < 2 or not np.isfinite(X).all():
        return bad
    _, dg = moments(X)
    if not np.isfinite(dg).all() or (dg <= 0).any():
        return bad
    sd, h, S = signs(X, c)
    A = np.abs(S)
    a = A.sum(axis=0)
    if (a == 0).any():
        return bad
    H = S.T @ S
    P = A.T @ A
    if variant == 2:
        G = H.astype(np.float64) / np.sqrt(np.outer(a, a).astype(np.float64))
    elif variant == 1:
        G = H.astype(np.float64) / (a[:, None] + a[None, :] - P).astype(np.float64)
    else:
        raise ValueError("variant must be 1 or 2")
    return Gerber(OK, sd, h, S, a, H, P, G, G * np.outer(sd, sd))


def margin(X, c):
    """min |(|x_tk| - h_k)| / h_k: how far, relative to the threshold, the closest entry of the
    window is from changing its sign class (a sign cannot depend on the last bits of sd where
    this is well above 1e-16)."""
    X = np.asarray(X, dtype=np.float64)
    _, h, _ = signs(X, c)
    return float(np.min(np.abs(np.abs(X) - h) / h))


def literal_counts(X, c):
    """N^UU, N^DD, N^UD, N^DU, N^NN by a literal double loop over the asset pairs and the days."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    _, h, _ = signs(X, c)
    N = {k: np.zeros((n, n), dtype=np.int64) for k in ("UU", "DD", "UD", "DU", "NN")}
    for i in range(n):
        for j in range(n):
            for t in range(T):
                ui, di = X[t, i] >= h[i], X[t, i] <= -h[i]
                uj, dj = X[t, j] >= h[j], X[t, j] <= -h[j]
                N["UU"][i, j] += ui and uj
                N["DD"][i, j] += di and dj
                N["UD"][i, j] += ui and dj
                N["DU"][i, j] += di and uj
                N["NN"][i, j] += (not ui and not di) and (not uj and not dj)
    return N
