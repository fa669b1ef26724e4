"""NumPy longdouble model of the exponentially weighted covariance as include/porqua_hip.h defines
it for pq_ewma_cov_batched.

For one T x n window X, oldest row first, and an age table wage (wage[k]: the weight of a row of
age k, the newest row has age 0):
    w_j = wage[T - 1 - j],  W1 = sum w,  W2 = sum w^2,  m = sum w_j x_j / W1,
    Sigma = sum_j w_j (x_j - m)(x_j - m)' / (W1 - W2 / W1)
-- np.cov(X, rowvar=False, aweights=w), and the last block of
DataFrame.ewm(halflife=h, adjust=True).cov(bias=False).  A window is bad input where T < 2, a value
is not finite or W1 - W2 / W1, evaluated in float64 as the kernel does, is not > 0.  The table is an
argument: the model never forms a power, so it and the device use the same float64 weights; all
sums are longdouble."""
from collections import namedtuple

import numpy as np

OK, BAD_INPUT = 0, 1
LD = np.longdouble

Ewma = namedtuple("Ewma", "status mean Sigma sd W1 den")


def den64(w):
    """W1 - W2 / W1 in float64, summed by increasing age as the kernel sums the table."""
    W1 = W2 = np.float64(0.0)
    for v in np.asarray(w, dtype=np.float64)[::-1]:
        W1 = W1 + v
        W2 = W2 + v * v
    with np.errstate(invalid="ignore", divide="ignore"):
        return W1 - W2 / W1


def ewma(X, wage):
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    bad = Ewma(BAD_INPUT, None, np.full((n, n), np.nan), None, None, None)
    if T < 2 or not np.isfinite(X).all():
        return bad
    w64 = np.asarray(wage, dtype=np.float64)[:T][::-1]   # oldest row first
    d64 = den64(w64)
    if not (np.isfinite(d64) and d64 > 0):
        return bad
    w = w64.astype(LD)
    W1, W2 = w.sum(), (w * w).sum()
    Xl = X.astype(LD)
    m = (w[:, None] * Xl).sum(axis=0) / W1
    Xc = Xl - m
    den = W1 - W2 / W1
    Sigma = (Xc * w[:, None]).T @ Xc / den
    return Ewma(OK, m, Sigma, np.sqrt(np.diag(Sigma)), W1, den)
