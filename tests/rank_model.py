"""NumPy model of the rank covariances (Spearman's rho, Kendall's tau-b) as include/porqua_hip.h
defines them for pq_rank_cov_batched.

For one complete T x n window X of finite doubles and asset k:
    d_tk = 2 #{u : x_uk < x_tk} + #{u : x_uk == x_tk} + 1   (the doubled mid-rank, IEEE < and ==),
    c_tk = d_tk - (T + 1);
    Spearman: C = c'c, rho_ij = C_ij / sqrt(C_ii C_jj);
    Kendall:  kappa_(s,t),k = sgn(x_tk - x_sk) for every pair of days s < t, H = kappa'kappa,
              tau_ij = H_ij / sqrt(H_ii H_jj)   (tau-b);
    m_k the window mean, dg_k = sum_t (x_tk - m_k)^2 (two passes), sd_k = sqrt(dg_k / (T - 1)),
    Sigma_ij = g_ij (sd_i sd_j), g = rho or tau.
A window is bad input where T < 2, a value is not finite or a column is constant (C_kk = H_kk = 0).
The counts are integers held in float64 (every product, sum and matmul below is exact: the largest
value, (T^3 - T) / 3 at T = 512, is 4.5e7), so BLAS forms them fast; the correlation is one square
root of a product and one division."""
from collections import namedtuple

import numpy as np

OK, BAD_INPUT = 0, 1
KINDS = ("spearman", "kendall")

Rank = namedtuple("Rank", "status counts diag corr Sigma sd")


def doubled_ranks(X):
    """d (int64 [T, n]) and eq (int64 [T, n], the number of days tied with day t, itself included)."""
    X = np.asarray(X, dtype=np.float64)
    lt = (X[None, :, :] < X[:, None, :]).sum(axis=1)
    eq = (X[None, :, :] == X[:, None, :]).sum(axis=1)
    return 2 * lt + eq + 1, eq


def pair_signs(X):
    """kappa (float64 [T (T - 1) / 2, n]): sgn(x_t - x_s) for every pair of days s < t."""
    X = np.asarray(X, dtype=np.float64)
    s, t = np.triu_indices(X.shape[0], k=1)
    return np.sign(X[t] - X[s])


def sd(X):
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    m = X.sum(axis=0) / T
    dg = ((X - m) ** 2).sum(axis=0)
    return np.sqrt(dg / (T - 1))


def rank_cov(X, kind="spearman"):
    if kind not in KINDS:
        raise ValueError("kind must be 'spearman' or 'kendall'")
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    nan = np.full((n, n), np.nan)
    bad = Rank(BAD_INPUT, None, None, nan, nan, None)
    if T < 2 or not np.isfinite(X).all():
        return bad
    if kind == "spearman":
        d, _ = doubled_ranks(X)
        c = (d - (T + 1)).astype(np.float64)
        counts = c.T @ c
    else:
        k = pair_signs(X)
        counts = k.T @ k
    diag = np.diag(counts).copy()
    if (diag == 0).any():
        return bad
    corr = counts / np.sqrt(np.outer(diag, diag))
    s = sd(X)
    return Rank(OK, counts, diag, corr, corr * np.outer(s, s), s)


def kendall_diag_from_ties(X):
    """H_kk = (T (T - 1) - sum_t (eq_tk - 1)) / 2: the pairs of days not tied in asset k, the
    form in which the ranking kernel computes the diagonal."""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    _, eq = doubled_ranks(X)
    return (T * (T - 1) - (eq - 1).sum(axis=0)) // 2
