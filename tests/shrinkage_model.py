"""Numpy yardsticks of the shrinkage-intensity kernel (pq_shrink_stats_band) and of the
``ledoit_wolf`` / ``oas`` covariance methods.

``stats`` is the model: in ``np.longdouble``, centre the window, K = Xc Xc', then
a = tr K, f = sum_st K_st^2, g = sum_t K_tt^2 and

    delta_LW  = clip((g - f/T) / (f - a^2/n), 0, 1)       (0 where the denominator is <= 0)
    delta_OAS = min(1, (f + a^2) / ((T+1) (f - a^2/n)))   (1 where the denominator is <= 0)

which are sklearn's ``ledoit_wolf_shrinkage(X)`` and ``oas(X)[1]`` rewritten through
||Xc'Xc||_F = ||Xc Xc'||_F and sum_t ||x_t||^4 = sum_t K_tt^2.  ``shrunk_cov`` is
Sigma* = (1 - delta) S + delta mean(diag S) I with the ddof = 1 sample covariance S.

``band_stats_f64`` restates the kernel's algorithm in float64 -- the uncentred Gram first,
centring from its row sums afterwards -- and sizes the bound of the conditioning test: its
error against the model is what that algorithm costs in float64, whatever the summation
order."""
import numpy as np

LD = np.longdouble
KINDS = ("ledoit_wolf", "oas")


def delta_from(a, f, g, T, n, kind):
    """The intensity from the three sums (any float type; T and n enter as floats)."""
    ft = type(a)
    T, n = ft(T), ft(n)
    den = f - a * a / n
    if kind == "ledoit_wolf":
        return min(max((g - f / T) / den, ft(0)), ft(1)) if den > 0 else ft(0)
    if kind == "oas":
        return min((f + a * a) / ((T + 1) * den), ft(1)) if den > 0 else ft(1)
    raise ValueError(kind)


def _sums(K):
    return np.trace(K), (K * K).sum(), (np.diag(K) ** 2).sum()


def gram(X):
    """X X' of a longdouble X (T x n, n <= 1024) in longdouble, without numpy's slow
    extended-precision matmul: X / scale is cut into three 21-bit integer pieces (63 bits below
    the largest entry, so X is reproduced to 2^-64 of it), every piece product is an integer
    below 2^42 and a sum of n <= 2^10 of them is exact in float64 in any order, so the nine
    float64 BLAS products are exact and only their longdouble combination rounds."""
    X = np.asarray(X, dtype=LD)
    assert X.shape[1] <= 1024
    top = np.abs(X).max()
    if top == 0:
        return np.zeros((X.shape[0],) * 2, dtype=LD)
    scale = LD(2) ** int(np.ceil(np.log2(float(top))) + 1)
    step = LD(2) ** 21
    pieces, r = [], X / scale
    for _ in range(3):
        r = r * step
        p = np.rint(r)
        pieces.append(p.astype(np.float64))
        r = r - p
    K = np.zeros((X.shape[0],) * 2, dtype=LD)
    for i, j in sorted(((i, j) for i in range(3) for j in range(3)), key=sum, reverse=True):
        K += (pieces[i] @ pieces[j].T).astype(LD) / step ** (i + j + 2)   # smallest terms first
    return K * scale * scale


def stats(X, kind="ledoit_wolf", centred=True):
    """(a, f, g, delta) of one window X (T x n) in longdouble."""
    X = np.asarray(X, dtype=LD)
    T, n = X.shape
    Xc = X - X.mean(axis=0) if centred else X
    a, f, g = _sums(gram(Xc))
    return a, f, g, delta_from(a, f, g, T, n, kind)


def shrunk_cov(X, kind="ledoit_wolf"):
    """(Sigma*, delta) in longdouble: (1 - delta) S + delta mean(diag S) I, S with ddof = 1."""
    X = np.asarray(X, dtype=LD)
    T, n = X.shape
    Xc = X - X.mean(axis=0)
    S = gram(Xc.T) / LD(T - 1)
    delta = stats(X, kind)[3]
    return (1 - delta) * S + delta * np.mean(np.diag(S)) * np.eye(n, dtype=LD), delta


def band_stats_f64(X, kind="ledoit_wolf", centred=True):
    """(a, f, g, delta) by the kernel's algorithm in float64: G = X X', c = row means of G,
    K = (G - c_s - c_t) + cbar, the sums from K's entries."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    K = X @ X.T
    if centred:
        c = K.sum(axis=1) / T
        K = (K - c[:, None] - c[None, :]) + c.sum() / T
    a, f, g = _sums(K)
    return a, f, g, delta_from(a, f, g, T, n, kind)
