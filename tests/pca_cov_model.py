"""NumPy float64 model of engine.pca_window_form for one window: the PCA factor covariance
(probabilistic PCA, Tipping & Bishop; sklearn's PCA.get_covariance()) from the eigenpairs of the
T x T Gram of the centred window, with a trace-preserving noise level.

    G = Xc Xc' = V diag(g) V',  l_j = g_j / (T - 1),  tr S = sum(Xc^2) / (T - 1)
    sigma2_k = (tr S - sum_{j<=k} l_j) / (n - k)
    Z_j = sqrt((1 - sigma2 / l_j) / (T - 1)) v_j' Xc,   Sigma = Z'Z + sigma2 I

``n_factors`` 'mp': the smallest k in 1..kmax with l_{k+1} <= (1 + sqrt(n / T))^2 sigma2_k (l_j = 0
beyond the Gram's size), kmax where none is."""
import numpy as np

OK, BAD_INPUT = 0, 1


class PcaModel:
    def __init__(self, status, k=0, sigma2=np.nan, evals=None, Z=None, Sigma=None, margin=np.inf):
        self.status, self.k, self.sigma2, self.evals, self.Z, self.Sigma = status, k, sigma2, evals, Z, Sigma
        self.margin = margin   # 'mp': the smallest |l_{k+1} - edge sigma2_k| / l_{k+1} over the steps examined


def pca_cov(X, n_factors="mp", kmax=64):
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    kcap = min(int(kmax), n - 1)
    if n_factors != "mp":
        if not 1 <= int(n_factors) <= kcap:
            raise ValueError("n_factors outside 1..min(kmax, n - 1)")
        kcap = int(n_factors)
    if T < 2:
        return PcaModel(BAD_INPUT)
    Xc = X - X.mean(0)
    G = Xc @ Xc.T
    if not np.all(np.isfinite(G)):
        return PcaModel(BAD_INPUT)
    g, V = np.linalg.eigh(G)
    g, V = g[::-1], V[:, ::-1]
    l = np.zeros(kcap + 1)
    m = min(T, kcap + 1)
    l[:m] = g[:m] / (T - 1)
    trS = (Xc * Xc).sum() / (T - 1)
    sig = (trS - np.cumsum(l[:kcap])) / (n - np.arange(1, kcap + 1))
    k, margin = kcap, np.inf
    if n_factors == "mp":
        edge = (1.0 + np.sqrt(n / T)) ** 2
        for kk in range(1, kcap + 1):
            if l[kk] > 0:
                margin = min(margin, abs(l[kk] - edge * sig[kk - 1]) / l[kk])
            if l[kk] <= edge * sig[kk - 1]:
                k = kk
                break
    sigma2 = sig[k - 1]
    gk = g[k - 1] if k <= T else 0.0
    if not gk > T * 2.0 ** -52 * g[0] or not sigma2 > 0 or not np.isfinite(sigma2):
        return PcaModel(BAD_INPUT, margin=margin)
    lk = l[:k]
    Z = np.sqrt((1.0 - sigma2 / lk) / (T - 1))[:, None] * (V[:, :k].T @ Xc)
    return PcaModel(OK, k, sigma2, lk, Z, Z.T @ Z + sigma2 * np.eye(n), margin)


def pca_cov_eigh(X, k):
    """The same Sigma by the n x n route: eigh of S = Xc'Xc / (T - 1), the top k pairs kept and
    the rest of the spectrum replaced by its mean over n - k."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    Xc = X - X.mean(0)
    S = Xc.T @ Xc / (T - 1)
    lam, U = np.linalg.eigh(S)
    lam, U = lam[::-1], U[:, ::-1]
    sigma2 = (np.trace(S) - lam[:k].sum()) / (n - k)
    return (U[:, :k] * (lam[:k] - sigma2)) @ U[:, :k].T + sigma2 * np.eye(n), sigma2
