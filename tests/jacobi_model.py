"""Independent models of jacobi.hip (TEST INFRASTRUCTURE ONLY): pq_sym_eig_batched,
pq_sym_eig_converged, pq_psd_form_batched and pq_tile_gemm_batched.

Two models of the eigensolver, for two different questions:

* ``jacobi_ref``: plain cyclic Jacobi in ``np.longdouble`` (u_ld = 2^-64), parallel
  (round-robin) ordering, one absolute rotation threshold, run until
  off(A) <= 1e-19 ||A||_F.  It shares nothing with the kernel but the textbook rotation and
  is the reference for eigenvalues: its own error is ~n u_ld ||A||, three orders below FP64's
  u = 2^-53.
* ``block_jacobi_f64``: the kernel's algebra in float64 -- the same block pairing (32-column
  blocks, round-robin rounds, 64 x 64 subproblems), the same cyclic Jacobi inside a
  subproblem with the same rotation rule, the same symmetrisation of the subproblem and the
  same two-sided tile updates.  It says what the kernel's *algorithm* loses in FP64
  (residual, orthogonality, eigenvalues, sweeps, convergence); the kernel may differ from it
  only by the order of its sums (MFMA tiles, fused multiply-adds).  It carries the same
  rotation rule as k_jac_pairs and must be changed with it:
      rotate (p, q) iff |a_pq| > tol sqrt|a_pp a_qq|  and  |a_pq| > tol u ||A||_F
                        and |a_pq| > 1e-300;
      a rotation whose sine rounds to 0 (tau^2 overflowed) is the identity and does not
      count as one.

``measures`` forms, in longdouble,
    resid = max|A V - V diag(lam)| / ||A||_F,  orth = max|V'V - I|,
    eig   = max|sort(lam) - sort(lam_ref)| / max|lam_ref|
(a zero denominator is replaced by 1: the zero matrix).

Product bars (u = 2^-53, all matrices ld x ld, S the elementwise sum of the magnitudes of the
terms, formed in longdouble):

* pq_tile_gemm_batched, C = op(A) op(B): every entry is a dot product of depth ld.  Each of
  the ld products is rounded once (or fused into the following addition) and the ld - 1
  additions once each, in any order, so |C - C_ref| <= gamma_ld S with
  gamma_ld = ld u / (1 - ld u) <= (ld + 1) u for ld u < 1/ (ld + 1)  ->  (ld + 1) u S.
* pq_psd_form_batched, out = sum_k (v_ik sqrt(l_k)) (v_jk sqrt(l_k)), l_k = max(lam_k, 0),
  k < n: on top of the dot product of depth ld every term carries the rounding of the
  sqrt, twice (it enters both factors), and the rounding of the two scalings
  v sqrt(l): four more factors (1 + delta)  ->  (ld + 5) u S with
  S = sum_k |v_ik| l_k |v_jk|.  (Terms must stay in the normal range: the cases use
  |l_k| >= 1e-200.)
"""
from __future__ import annotations

import zlib

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
assert np.finfo(LD).eps < 1e-18, "jacobi_ref needs an extended-precision long double"

JB, JS = 32, 64


# ----------------------------------------------------------------------------
# round-robin pairing (circle method), as in jacobi.hip
# ----------------------------------------------------------------------------

def rr_member(k, r, nb):
    return 0 if k == 0 else ((k - 1 + r) % (nb - 1)) + 1


def rr_pair(i, r, nb):
    a, b = rr_member(i, r, nb), rr_member(nb - 1 - i, r, nb)
    return (a, b) if a < b else (b, a)


def _rr_steps(m):
    """[(p[], q[]) for each of the m - 1 steps]: m / 2 disjoint pairs p < q per step (m even)."""
    out = []
    for step in range(m - 1):
        pq = [rr_pair(k, step, m) for k in range(m // 2)]
        out.append((np.array([a for a, _ in pq]), np.array([b for _, b in pq])))
    return out


_STEPS64 = _rr_steps(JS)


def _rotate(S, Ws, p, q, c, s):
    """S <- G' S G, every W in Ws <- W G for the disjoint rotations (p, q, c, s):
    row_p' = c row_p - s row_q, row_q' = s row_p + c row_q, the same on the columns."""
    cr, sr = c[:, None], s[:, None]
    a, b = S[p, :].copy(), S[q, :].copy()
    S[p, :] = cr * a - sr * b
    S[q, :] = sr * a + cr * b
    a, b = S[:, p].copy(), S[:, q].copy()
    S[:, p] = c * a - s * b
    S[:, q] = s * a + c * b
    for W in Ws:
        a, b = W[:, p].copy(), W[:, q].copy()
        W[:, p] = c * a - s * b
        W[:, q] = s * a + c * b
    S[p, q] = 0.0
    S[q, p] = 0.0


# ----------------------------------------------------------------------------
# the high-precision reference
# ----------------------------------------------------------------------------

def jacobi_ref(A, max_sweeps=80):
    """Eigenvalues and eigenvectors (columns) of the symmetric A by cyclic Jacobi in
    longdouble -> (lam[n], V[n, n]), unsorted; off(A) <= 1e-19 ||A||_F on return."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    A = (A + A.T) / 2
    V = np.eye(n, dtype=LD)
    mx = np.abs(A).max() if n else LD(0)
    if n < 2 or mx == 0:
        return np.diag(A).copy(), V
    fro = mx * np.sqrt(np.sum((A / mx) ** 2))
    goal = LD("1e-19") * fro
    thr = goal / n                                   # every entry below thr: off <= n thr = goal
    m = n + (n & 1)
    steps = _rr_steps(m)
    for _ in range(max_sweeps):
        off2 = (A / mx) ** 2
        np.fill_diagonal(off2, 0)                    # not sum - diagonal: that cancels
        off = mx * np.sqrt(np.sum(off2))
        if off <= goal:
            return np.diag(A).copy(), V
        for p, q in steps:
            keep = q < n
            p, q = p[keep], q[keep]
            apq = A[p, q]
            rot = np.abs(apq) > thr
            if not rot.any():
                continue
            p, q, apq = p[rot], q[rot], apq[rot]
            tau = (A[q, q] - A[p, p]) / (2 * apq)
            t = np.where(tau >= 0, LD(1), LD(-1)) / (np.abs(tau) + np.hypot(LD(1), tau))
            c = 1 / np.hypot(LD(1), t)
            _rotate(A, [V], p, q, c, t * c)
    raise RuntimeError("jacobi_ref did not converge")


# ----------------------------------------------------------------------------
# the kernel's algebra in float64
# ----------------------------------------------------------------------------

def fro_scaled(A):
    """||A||_F as k_jac_scale forms it: scaled by the largest magnitude."""
    m = float(np.abs(A).max()) if A.size else 0.0
    if not (0.0 < m < np.inf):
        return m
    return m * float(np.sqrt(np.sum((A / m) ** 2)))


def _rule(apq, app, aqq, tol, floor):
    a = np.abs(apq)
    return (a > tol * np.sqrt(np.abs(app) * np.abs(aqq))) & (a > floor) & (a > 1e-300)


def _sub_jacobi(S, tol, floor):
    """Cyclic Jacobi on one 64 x 64 subproblem (k_jac_pairs) -> (W, rotated)."""
    W = np.eye(JS)
    any_rot = False
    d = np.arange(JS)
    for _ in range(30):
        dg = np.abs(np.diag(S))
        todo = _rule(S, dg[:, None], dg[None, :], tol, floor)
        todo[d, d] = False
        if not todo.any():                           # a sweep over this S rotates nothing
            break
        swept = False
        for p, q in _STEPS64:
            apq = S[p, q]
            rot = _rule(apq, S[p, p], S[q, q], tol, floor)
            if not rot.any():
                continue
            pr, qr, apq = p[rot], q[rot], apq[rot]
            with np.errstate(over="ignore"):
                tau = (S[qr, qr] - S[pr, pr]) / (2.0 * apq)
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            real = s != 0.0
            if not real.any():
                continue
            swept = True
            _rotate(S, [W], pr[real], qr[real], c[real], s[real])
        if not swept:
            break
        any_rot = True
    return W, any_rot


def block_jacobi_f64(A, n, ld, max_sweeps=30, tol=1e-14):
    """pq_sym_eig_batched on one matrix, in float64 -> (evals[ld], V[ld, ld], sweeps_used,
    converged).  sweeps_used counts the sweeps that ran, the one that rotated nothing
    included (1: nothing was ever rotated); converged as pq_sym_eig_converged reports it."""
    W = np.zeros((ld, ld))
    W[:n, :n] = np.asarray(A, dtype=np.float64)[:n, :n]
    V = np.eye(ld)
    floor = tol * U * fro_scaled(W[:n, :n])
    nbk = ld // JB
    npairs, nrounds = nbk // 2, nbk - 1
    sweeps, converged = 0, False
    for _ in range(max_sweeps):
        sweeps += 1
        any_s = False
        for r in range(nrounds):
            idx, rots, flags = [], [], []
            for i in range(npairs):
                bi, bj = rr_pair(i, r, nbk)
                ix = np.concatenate([np.arange(bi * JB, (bi + 1) * JB), np.arange(bj * JB, (bj + 1) * JB)])
                blk = W[np.ix_(ix, ix)]
                Wp, rot = _sub_jacobi(0.5 * (blk + blk.T), tol, floor)
                idx.append(ix), rots.append(Wp), flags.append(rot)
            for P in range(npairs):                 # every tile reads and writes itself only
                for Q in range(npairs):
                    if flags[P] or flags[Q]:
                        sel = np.ix_(idx[P], idx[Q])
                        W[sel] = rots[P].T @ (W[sel] @ rots[Q])
            for Q in range(npairs):
                if flags[Q]:
                    V[:, idx[Q]] = V[:, idx[Q]] @ rots[Q]
            any_s = any_s or any(flags)
        if not any_s:
            converged = True
            break
    return np.diag(W).copy(), V, sweeps, converged


# ----------------------------------------------------------------------------
# measures and product references (longdouble)
# ----------------------------------------------------------------------------

def measures(A, evals, V, n, lam_ref=None):
    """(resid, orth, eig) of the eigenpairs (evals[:n], V[:n, :n]) of A[:n, :n]."""
    A = np.asarray(A, dtype=LD)[:n, :n]
    lam = np.asarray(evals, dtype=LD)[:n]
    V = np.asarray(V, dtype=LD)[:n, :n]
    if lam_ref is None:
        lam_ref = jacobi_ref(A)[0]
    mx = np.abs(A).max()
    fro = mx * np.sqrt(np.sum((A / mx) ** 2)) if mx > 0 else LD(1)
    resid = np.abs(A @ V - V * lam[None, :]).max() / fro
    orth = np.abs(V.T @ V - np.eye(n, dtype=LD)).max()
    top = np.abs(lam_ref).max()
    eig = np.abs(np.sort(lam) - np.sort(np.asarray(lam_ref, dtype=LD))).max() / (top if top > 0 else LD(1))
    return float(resid), float(orth), float(eig)


def psd_form_ref(V, evals, n):
    """out = V[:, :n] diag(max(evals[:n], 0)) V[:, :n]' and S = |V| diag(.) |V|' (ld x ld)."""
    Vl = np.asarray(V, dtype=LD)[:, :n]
    lam = np.maximum(np.asarray(evals, dtype=LD)[:n], 0)
    return (Vl * lam) @ Vl.T, (np.abs(Vl) * lam) @ np.abs(Vl).T


def gemm_ref(A, ta, B, tb):
    """op(A) op(B) and S = |op(A)| |op(B)|."""
    A = np.asarray(A, dtype=LD)
    B = np.asarray(B, dtype=LD)
    A = A.T if ta else A
    B = B.T if tb else B
    return A @ B, np.abs(A) @ np.abs(B)


# ----------------------------------------------------------------------------
# the named matrices
# ----------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _sym(M):
    return 0.5 * (M + M.T)


def _cov(X):
    Xc = X - X.mean(axis=0)
    return _sym(Xc.T @ Xc / (X.shape[0] - 1))


def round_up(n, m):
    return (n + m - 1) // m * m


def matrix(name, n):
    """The matrix called ``name`` at size n (seeded by both)."""
    r = _rng(name, n)
    T = max(n // 3, 2)
    if name == "gauss":
        return _sym(r.normal(size=(n, n)))
    if name == "gauss_1e-150":
        return _sym(r.normal(size=(n, n))) * 1e-150
    if name == "gauss_1e150":
        return _sym(r.normal(size=(n, n))) * 1e150
    if name == "cov":
        return _cov(r.normal(0, 0.02, size=(T, n)))
    if name == "negcov":
        return -_cov(r.normal(0, 0.02, size=(T, n)))
    if name == "diagonal":
        return np.diag(r.normal(size=n))
    if name == "0.3I":
        return 0.3 * np.eye(n)
    if name == "zero":
        return np.zeros((n, n))
    if name == "I+rank1":
        v = r.normal(size=n)
        return 0.3 * np.eye(n) + np.outer(v, v)
    if name == "ones":
        return np.ones((n, n))
    if name == "block_ones":
        A = np.zeros((n, n))
        A[:40, :40] = 1.0
        return A
    if name == "rank2":
        v, w = r.normal(size=(2, n))
        return np.outer(v, v) + np.outer(w, w)
    if name == "dupcols":
        X = r.normal(0, 0.02, size=(T, n))
        X[:, n // 2:] = X[:, :n - n // 2]
        return _cov(X)
    if name == "constcol":
        X = r.normal(0, 0.02, size=(T, n))
        X[:, 3 % n] = 0.5                            # exact mean: an exact zero row and column
        return _cov(X)
    if name == "graded":
        Q, _ = np.linalg.qr(r.normal(size=(n, n)))
        return _sym((Q * np.logspace(0, -14, n)) @ Q.T)
    if name == "ring":
        A = np.zeros((n, n))
        i = np.arange(n)
        A[i, (i + 1) % n] = 1.0
        A[(i + 1) % n, i] = 1.0
        return A
    if name == "tiny_coupling":                      # [[0, 1e-200], [1e-200, 1]] on (0, n - 1)
        A = np.zeros((n, n))
        A[n - 1, n - 1] = 1.0
        A[0, n - 1] = A[n - 1, 0] = 1e-200
        return A
    raise KeyError(name)


SPECTRA = ["gauss", "cov", "negcov", "diagonal", "0.3I", "zero", "I+rank1", "ones", "rank2", "dupcols",
           "constcol", "gauss_1e-150", "gauss_1e150"]
NOTHING_TO_ROTATE = {"diagonal", "0.3I", "zero", "tiny_coupling"}


def cases():
    """[(name, n, ld, A)]: every spectrum at n = 65 and 97 (ld 128), the sized ones, the three
    that run at n = 129 (ld 192), and the pairing / padding edges on gauss."""
    out = []
    for n in (65, 97):
        out += [(s, n, 128) for s in SPECTRA]
    out += [("graded", 97, 128), ("block_ones", 70, 128), ("ring", 64, 64), ("ring", 97, 128),
            ("tiny_coupling", 2, 64), ("tiny_coupling", 66, 128)]
    out += [(s, 129, 192) for s in ("gauss", "cov", "I+rank1")]
    out += [("gauss", n, 64) for n in (1, 2, 31, 32, 33, 63, 64)]
    out += [("gauss", n, 128) for n in (96, 128)] + [("cov", 64, 64), ("cov", 128, 128)]
    out += [("gauss", 10, 128)]
    return [(name, n, ld, matrix(name, n)) for name, n, ld in out]
