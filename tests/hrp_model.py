"""Extended-precision model of hierarchical risk parity (Lopez de Prado 2016), independent of
the engine, in np.longdouble on the dense Sigma:

1. rho_ij = Sigma_ij / sqrt(Sigma_ii Sigma_jj) clipped to [-1, 1], D_ij = sqrt((1 - rho_ij) / 2);
2. the single-linkage tree with SciPy's conventions: Prim's minimum spanning tree from asset 0
   (``best`` updated on strict <, the lowest index among the minima joins next), the n - 1 edges
   stably sorted by distance, merged by a union-find (merge k creates cluster n + k, its children
   the current roots of the edge's ends, the smaller id first);
3. the leaves in pre-order, first child before second (an explicit stack);
4. recursive bisection of the ordered list into its first L // 2 and remaining entries, each pair
   sharing its weight by the inverse-variance cluster variances v = u' Sigma_cc u.

``hrp`` is the model; ``hrp_f64`` restates what the kernel does in float64 numpy (Sigma formed
as alpha S + c I from a float64 S, the order taken on 1 - rho, the cluster variances assembled
bottom-up from the cross blocks of the bisection tree); the tests measure its distance from the
model to size their tolerances.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble


def correlation(S):
    S = np.asarray(S, dtype=LD)
    sd = np.sqrt(np.diag(S))
    return np.clip(S / np.outer(sd, sd), LD(-1), LD(1))


def distance(S):
    D = np.sqrt((LD(1) - correlation(S)) / LD(2))
    np.fill_diagonal(D, LD(0))
    return D


def prim_edges(D):
    """Prim's tree from vertex 0 on the dense distance (or any monotone key) matrix:
    (a [n-1], b [n-1], d [n-1]) in insertion order, a the tree-side end (the vertex ``best`` came
    from) and b the vertex that joined."""
    n = D.shape[0]
    merged = np.zeros(n, dtype=bool)
    best = np.full(n, np.inf, dtype=D.dtype)
    src = np.zeros(n, dtype=np.int64)
    a, b, d = (np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1, dtype=np.int64), np.zeros(n - 1, dtype=D.dtype))
    x = 0
    for k in range(n - 1):
        merged[x] = True
        upd = ~merged & (D[x] < best)          # strict <
        best[upd] = D[x][upd]
        src[upd] = x
        cand = np.where(merged, np.inf, best)
        y = int(np.argmin(cand))               # the lowest index among the minima
        a[k], b[k], d[k] = src[y], y, best[y]
        x = y
    return a, b, d


def label(a, b, d):
    """Stable sort by distance, then the union-find merges -> Z [n-1, 4] in SciPy's layout
    (child, child, distance, size), in d's dtype."""
    m = len(d)
    n = m + 1
    perm = np.argsort(d, kind="stable")
    parent = np.arange(2 * n - 1)
    size = np.ones(2 * n - 1, dtype=np.int64)

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:                  # path compression
            parent[v], v = r, parent[v]
        return r

    Z = np.zeros((m, 4), dtype=d.dtype)
    for k, e in enumerate(perm):
        ra, rb = find(a[e]), find(b[e])
        parent[ra] = parent[rb] = n + k
        size[n + k] = size[ra] + size[rb]
        Z[k] = (min(ra, rb), max(ra, rb), d[e], size[n + k])
    return Z


def leaves(Z, n):
    """Pre-order leaves from the root, first child before second, with an explicit stack."""
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    out = []
    stack = [2 * n - 2]
    while stack:
        v = stack.pop()
        if v < n:
            out.append(v)
        else:
            stack.append(int(Z[v - n, 1]))
            stack.append(int(Z[v - n, 0]))
    return np.array(out, dtype=np.int64)


def cluster_var(S, idx):
    Sc = S[np.ix_(idx, idx)]
    u = 1 / np.diag(Sc)
    u = u / u.sum()
    return u @ (Sc @ u)


def bisect(S, order):
    """The weights (sum 1, indexed by asset) of the recursive bisection of ``order``."""
    n = len(order)
    w = np.ones(n, dtype=S.dtype)
    lists = [np.asarray(order)]
    while lists:
        nxt = []
        for c in lists:
            L = len(c)
            if L < 2:
                continue
            left, right = c[:L // 2], c[L // 2:]
            vl, vr = cluster_var(S, left), cluster_var(S, right)
            alpha = 1 - vl / (vl + vr)
            w[left] *= alpha
            w[right] *= 1 - alpha
            nxt += [left, right]
        lists = nxt
    return w


def min_gap(Z):
    """The smallest gap between consecutive sorted merge distances (+inf for n <= 2)."""
    d = np.asarray(Z[:, 2])
    return float(np.min(np.diff(d))) if len(d) > 1 else float("inf")


def hrp(S, scale=1.0):
    """The model: (x [n], order [n], Z [n-1, 4], stats = (x' Sigma x, min gap)), longdouble."""
    S = np.asarray(S, dtype=LD)
    n = S.shape[0]
    if n == 1:
        x = np.array([LD(scale)])
        return x, np.zeros(1, dtype=np.int64), np.zeros((0, 4), dtype=LD), (float(x[0] * x[0] * S[0, 0]), float("inf"))
    Z = label(*prim_edges(distance(S)))
    order = leaves(Z, n)
    x = LD(scale) * bisect(S, order)
    return x, order, Z, (float(x @ (S @ x)), min_gap(Z))


def pairwise_gap(S):
    """The smallest gap between two DISTINCT pairwise distances of the model (inf if all tie)."""
    D = distance(S)
    d = np.unique(D[np.triu_indices(D.shape[0], 1)])
    return float(np.min(np.diff(d))) if len(d) > 1 else float("inf")


# ---- the float64 restatement of the kernel ----------------------------------------------------

def _tree_nodes(n):
    """The bisection tree over positions 0..n-1 in heap numbering: {h: (lo, hi)}, root 1,
    children 2h (the first L // 2 positions) and 2h + 1."""
    nodes = {}
    stack = [(1, 0, n)]
    while stack:
        h, lo, hi = stack.pop()
        nodes[h] = (lo, hi)
        if hi - lo > 1:
            mid = lo + (hi - lo) // 2
            stack += [(2 * h, lo, mid), (2 * h + 1, mid, hi)]
    return nodes


def hrp_f64(S, alpha, c, scale=1.0):
    """float64, as the kernel computes: d = alpha S_ii + c, rho_ij = (alpha S_ij) (isd_i isd_j)
    with isd = 1 / sqrt(d), the tree on the key 1 - rho, distances sqrt(key / 2) only where they
    are reported; Q_c = iv' Sigma_cc iv (iv = 1 / d) bottom-up over the bisection tree from the
    cross blocks, v_c = Q_c / (sum iv)^2; x' Sigma x from the diagonal and the same cross blocks."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    alpha, c, scale = float(alpha), float(c), float(scale)
    d = alpha * np.diag(S) + c
    if n == 1:
        x = np.array([scale])
        return x, np.zeros(1, dtype=np.int64), np.zeros((0, 4)), (float(x[0] * x[0] * d[0]), float("inf"))
    isd = 1.0 / np.sqrt(d)
    key = 1.0 - np.clip((alpha * S) * np.outer(isd, isd), -1.0, 1.0)
    a, b, k = prim_edges(key)
    Z = label(a, b, k)
    Z[:, 2] = np.sqrt(0.5 * Z[:, 2])
    order = leaves(Z, n)
    iv = (1.0 / d)[order]
    So = alpha * S[np.ix_(order, order)]
    nodes = _tree_nodes(n)
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
    return x, order, Z, (scale * scale * var, min_gap(Z))


# ---- the windows the GPU test runs, shared with the CPU test of their conditions --------------

NS = (1, 2, 3, 5, 16, 17, 37, 64, 65, 130, 257)
TS = (7, 63, 252)
RIDGE = 2e-5          # the c > 0 cases (the assets' variances are about 5e-4)
GAP_MIN = 1e-11       # the smallest gap between distinct pairwise distances a window may have
# The row table of a case is tests/test_shrinkage_gpu._row_table(T) on the panel rows 9...; where
# one of its windows has two distinct pairwise distances closer than GAP_MIN, the whole table is
# moved to the rows 400... (n = 257, T = 252: the weekend-skipping date has a gap of 3.0e-13 at 9...)
SHIFT = {(257, 252): 391}


def case_rows(n, T):
    from tests.test_shrinkage_gpu import _row_table
    rows, lens = _row_table(T)
    return np.where(rows >= 0, rows + SHIFT.get((n, T), 0), rows).astype(np.int32), lens


def case_alpha(lens):
    """Sigma = alpha X_c'X_c + c I: the sample covariance (a one-row window keeps alpha = 1)."""
    return 1.0 / np.maximum(np.asarray(lens) - 1, 1).astype(np.float64)


def gram(R, rows):
    """X_c'X_c of the window in float64 (numpy; the GPU test forms it with torch)."""
    X = np.asarray(R, dtype=np.float64)[np.asarray(rows, dtype=np.int64)]
    Xc = X - X.mean(axis=0)
    return Xc.T @ Xc


def sigma(S, alpha, c):
    """alpha S + c I in longdouble from a float64 S, or None where its diagonal is not positive
    (the date is bad input)."""
    S = np.asarray(S, dtype=np.float64)
    Sig = LD(alpha) * S.astype(LD) + LD(c) * np.eye(S.shape[0], dtype=LD)
    return Sig if np.all(np.diag(Sig) > 0) else None


def deviation(S, alpha, c, scale, ref=None):
    """Relative deviations of hrp_f64 from the model on one date: (x, link distances, x' Sigma x),
    None if the trees differ."""
    x, order, Z, st = hrp(sigma(S, alpha, c), scale) if ref is None else ref
    xf, of, Zf, sf = hrp_f64(S, alpha, c, scale)
    if not (np.array_equal(of, order) and np.array_equal(Zf[:, [0, 1, 3]], np.asarray(Z[:, [0, 1, 3]], dtype=np.float64))):
        return None
    ex = float(np.max(np.abs(xf - x) / x))
    ed = float(np.max(np.abs(Zf[:, 2] - Z[:, 2]) / Z[:, 2])) if len(Z) and np.all(Z[:, 2] > 0) else 0.0
    return ex, ed, abs(sf[0] - st[0]) / st[0]
