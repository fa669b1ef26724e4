"""Model of hierarchical risk parity on SciPy's complete, average, weighted and Ward trees,
independent of the engine: the nearest-neighbour chain with a Lance-Williams update of the full
distance matrix, in plain numpy and generic in the dtype.

* An empty chain starts at the lowest live index.  From the chain's top x the candidate is the
  previous element y (``current_min`` = D[x, y]; +inf for a chain of one); a live i != x replaces
  it only on strict <, i upward, so the lowest index among strictly smaller minima wins and the
  previous element wins ties.  The previous element merges with x; anything else is pushed.
* A merge pops both, orders them x < y, records (x, y, current_min), retires slot x and stores in
  slot y the update against every live i, in the operation order of SciPy's
  _hierarchy_distance_update.pxi.
* The merges are stably sorted by distance and labelled by tests/hrp_model.label: a union-find
  over the recorded slots, the smaller root first, the sizes the union-find's (on an all-ties
  matrix they differ from the chain's).

``hrp`` runs it in longdouble on hrp_model.distance(Sigma): the reference.  ``hrp_f64`` runs it in
float64 on the D the kernel forms -- hrp_model.hrp_f64's key from the upper triangle of S,
D = sqrt(key / 2), mirrored -- followed by the kernel's bisection: the restatement, whose distance
from the reference sizes the tolerances of tests/test_hrp_linkage_gpu.py.
"""
from __future__ import annotations

import numpy as np

from tests import hrp_model as m

LD = m.LD
METHODS = ("complete", "average", "weighted", "ward")


def update(method, dxi, dyi, dxy, nx, ny, ni):
    """The new distance of cluster i to the merged x and y; sizes in the distances' dtype."""
    if method == "complete":
        return np.maximum(dxi, dyi)
    if method == "average":
        return (nx * dxi + ny * dyi) / (nx + ny)
    if method == "weighted":
        return (dxi + dyi) / 2
    if method == "ward":
        t = 1 / (nx + ny + ni)
        return np.sqrt((ni + nx) * t * dxi * dxi + (ni + ny) * t * dyi * dyi - ni * t * dxy * dxy)
    raise ValueError(method)


def nn_chain(D, method):
    """(x [n-1], y [n-1], d [n-1]) of the merges in chain order, x < y the slots, in D's dtype."""
    D = np.array(D)                                # a copy: the updates are in place
    dt = D.dtype.type
    n = D.shape[0]
    inf = dt(np.inf)
    size = np.zeros(n, dtype=np.int64) + 1
    xs, ys, ds = np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1, dtype=D.dtype)
    chain = []
    for k in range(n - 1):
        if not chain:
            chain = [int(np.flatnonzero(size > 0)[0])]
        while True:
            x = chain[-1]
            y, cur = (chain[-2], D[x, chain[-2]]) if len(chain) > 1 else (-1, inf)
            row = np.where(size > 0, D[x], inf)
            row[x] = inf
            i = int(np.argmin(row))                # the lowest index among the minima
            if row[i] < cur:                       # strict <
                y, cur = i, row[i]
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = size[x], size[y]
        xs[k], ys[k], ds[k] = x, y, cur
        size[x], size[y] = 0, nx + ny
        live = size > 0
        live[y] = False
        new = update(method, D[x, live], D[y, live], cur, dt(nx), dt(ny), size[live].astype(D.dtype))
        D[y, live] = new
        D[live, y] = new
    return xs, ys, ds


def tree(D, method):
    """Z [n-1, 4] in SciPy's layout and D's dtype."""
    return m.label(*nn_chain(D, method))


def hrp(S, method, scale=1.0):
    """The model: (x [n], order [n], Z [n-1, 4], stats = (x' Sigma x, min gap)), longdouble."""
    S = np.asarray(S, dtype=LD)
    n = S.shape[0]
    if n == 1:
        return m.hrp(S, scale)
    Z = tree(m.distance(S), method)
    order = m.leaves(Z, n)
    x = LD(scale) * m.bisect(S, order)
    return x, order, Z, (float(x @ (S @ x)), m.min_gap(Z))


def kernel_distance(S, alpha, c):
    """The D the kernel writes: d = alpha S_ii + c, key_ij = 1 - clip((alpha S_ij)(isd_i isd_j)) with
    isd = 1 / sqrt(d), D_ij = sqrt(key_ij / 2) from the upper triangle of S, mirrored, diagonal 0."""
    S = np.asarray(S, dtype=np.float64)
    isd = 1.0 / np.sqrt(float(alpha) * np.diag(S) + float(c))
    key = 1.0 - np.clip((float(alpha) * S) * np.outer(isd, isd), -1.0, 1.0)
    U = np.triu(np.sqrt(0.5 * key), 1)
    return U + U.T


def bisect_f64(S, alpha, c, order, scale):
    """The kernel's bisection of ``order`` in float64, as hrp_model.hrp_f64 states it: Q_c bottom-up
    over the bisection tree from the cross blocks, x' Sigma x from the diagonal and the same blocks.
    Returns (x by asset, x' Sigma x)."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    d = alpha * np.diag(S) + c
    iv = (1.0 / d)[order]
    So = alpha * S[np.ix_(order, order)]
    nodes = m._tree_nodes(n)
    Q, siv, al = {}, {}, {}
    for h in sorted(nodes, reverse=True):
        lo, hi = nodes[h]
        if hi - lo == 1:
            Q[h] = siv[h] = iv[lo]
            continue
        mid = lo + (hi - lo) // 2
        X = float(np.sum(iv[lo:mid] * (So[lo:mid, mid:hi] @ iv[mid:hi])))
        Q[h] = (Q[2 * h] + Q[2 * h + 1]) + 2.0 * X
        siv[h] = siv[2 * h] + siv[2 * h + 1]
        vl = Q[2 * h] / (siv[2 * h] * siv[2 * h])
        vr = Q[2 * h + 1] / (siv[2 * h + 1] * siv[2 * h + 1])
        al[h] = 1.0 - vl / (vl + vr)
    w = np.ones(n)
    for p in range(n):
        h, lo, hi = 1, 0, n
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            if p < mid:
                w[p] *= al[h]
                h, hi = 2 * h, mid
            else:
                w[p] *= 1.0 - al[h]
                h, lo = 2 * h + 1, mid
    var = float(np.sum(w * w / iv))
    for h, (lo, hi) in nodes.items():
        if hi - lo > 1:
            mid = lo + (hi - lo) // 2
            var += 2.0 * float(np.sum(w[lo:mid] * (So[lo:mid, mid:hi] @ w[mid:hi])))
    x = np.zeros(n)
    x[order] = scale * w
    return x, scale * scale * var


def hrp_f64(S, alpha, c, method, scale=1.0):
    """float64, as the kernel computes: the chain on kernel_distance, then bisect_f64."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    alpha, c, scale = float(alpha), float(c), float(scale)
    if n == 1:
        return m.hrp_f64(S, alpha, c, scale)
    Z = tree(kernel_distance(S, alpha, c), method)
    order = m.leaves(Z, n)
    x, var = bisect_f64(S, alpha, c, order, scale)
    return x, order, Z, (var, m.min_gap(Z))


def same_tree(A, B):
    """Children, sizes and leaf order of two (x, order, Z, stats) results are equal."""
    return (np.array_equal(A[1], B[1])
            and np.array_equal(np.asarray(A[2][:, [0, 1, 3]], dtype=np.float64),
                               np.asarray(B[2][:, [0, 1, 3]], dtype=np.float64)))


def deviation(ref, got):
    """Relative deviations (x, link distances, x' Sigma x) of one result from a reference of the
    same tree."""
    x, _, Z, st = ref
    xf, _, Zf, sf = got
    ex = float(np.max(np.abs(xf - x) / x))
    ed = float(np.max(np.abs(Zf[:, 2] - Z[:, 2]) / Z[:, 2])) if len(Z) and np.all(Z[:, 2] > 0) else 0.0
    return ex, ed, abs(sf[0] - st[0]) / st[0]


# ---- the windows the GPU test runs, shared with the CPU test of their conditions --------------

N_BIG, T_BIG = 1024, 63   # PQ_HRP_NMAX: the panel rows 9 .. 9 + T_BIG - 1, alpha = 1 / (T_BIG - 1)
# The row tables are hrp_model.case_rows', its SHIFT included: no method's longdouble tree differs
# from the restatement's on any of their windows but the one below, so none had to be moved further.


def is_scaled_identity(S):
    """Sigma = c I: S = 0, the one-row window (with the ridge; without it the date is bad input).
    Every distance is exactly sqrt(1 / 2) there, and for n >= 16 the rounding of the average and
    Ward updates decides the ties: these dates are compared against the float64 model, not the
    longdouble one."""
    return not np.any(S)


def big_rows():
    return np.arange(9, 9 + T_BIG, dtype=np.int32)
