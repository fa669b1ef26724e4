# Host-side API restatement of PorQua (part of the GeomScale project; reference tree
# amolrpatil21/PorQua): src/covariance.py.  PorQua is Copyright (c) 2024 Cyril Bachelard and
# Minh Ha Ho and licensed under the GNU LGPL v3; this module keeps that API and its
# behaviour (quirks included) so that the MI355X engine is a drop-in, and is distributed
# under the same licence terms.
"""Covariance estimation on the device (mirror of src/covariance.py:21-84).

``Covariance.estimate(X)`` keeps the reference signature (T x n DataFrame in, n x n
DataFrame out) and computes the two-pass np.cov / DataFrame.cov() result with K1
(window mean + FP64-MFMA SYRK; windows with NaN: pandas' pairwise-complete covariance from
four masked MFMA Grams), the PD check with K2's Cholesky info and the repair with
``helper_functions.nearestPD``.  Beyond the reference's methods, 'ledoit_wolf' and 'oas' shrink
towards mean(diag S) I with a data-driven intensity per window (engine.shrinkage_intensity:
three sums over the window's T x T Gram), and 'pca' is the statistical factor model
(probabilistic PCA, sklearn's PCA.get_covariance()): the top ``n_factors`` principal components
of the window kept, the rest of the spectrum replaced by one trace-preserving noise level
(engine.pca_window_form), and 'gerber' is the Gerber statistic (Gerber et al. 2022; Riskfolio-Lib's
gerber1 / gerber2): co-movement counts of the raw returns beyond ``threshold`` window standard
deviations in place of the second moments (engine.gerber_cov; spec ``threshold`` 0.5 and
``variant`` 2 by default), and 'spearman' / 'kendall' are the rank correlations -- Spearman's rho
and Kendall's tau-b of the window's columns, with mid-ranks for ties -- scaled by the window's
standard deviations (engine.rank_cov), and 'ewma' is the exponentially weighted covariance
(RiskMetrics 1996; np.cov(aweights=), pandas' ewm().cov()) with spec ``halflife`` or ``decay``
(engine.ewma_cov).  ``estimate_batch`` is the batched backtest entry: all
rebalance dates of a device-resident panel at once, results left on the device.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from .helper_functions import isPD, nearestPD


class CovarianceSpecification(dict):
    """Defaults: method 'pearson', check_positive_definite True (src/covariance.py:21-28)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self
        self.setdefault("method", "pearson")
        if self.get("method") is None:
            self["method"] = "pearson"
        if self.get("check_positive_definite") is None:
            self["check_positive_definite"] = True


def _shrink_lambda(lam):
    if lam is None or np.isnan(lam) or lam < 0:
        return 0.0
    return float(lam)


# data-driven shrinkage towards mean(diag S) I: Sigma* = (1 - delta) S + delta mean(diag S) I
SHRINKAGE_METHODS = ("ledoit_wolf", "oas")
# rank correlations scaled by the window's standard deviations (engine.rank_cov)
RANK_METHODS = ("spearman", "kendall")
# methods estimated per date from the date's own window, as a dense matrix only: no window form
# that dates could share (estimate_batch_lr serves them with materialise=True only)
DENSE_ONLY_METHODS = ("gerber",) + RANK_METHODS + ("ewma",)


class Covariance:
    """``shrinkage_``: the intensity delta of the last ``estimate`` with a SHRINKAGE_METHODS
    method (float); ``shrinkage_batch_``: the (B,) device tensor of the last batched estimate
    with one, None after any other method.

    method 'pca' (spec ``n_factors``: an int k, 1 <= k <= min(64, n - 1), or 'mp', the default:
    the Marchenko-Pastur count of engine.pca_window_form): ``n_factors_`` and ``noise_variance_``
    hold the factor count and the noise level sigma2 of the last ``estimate``;
    ``n_factors_batch_`` / ``noise_variance_batch_`` the (B,) device tensors of the last
    ``window_form_pca``.  The estimate is Z'Z + sigma2 I with k factor rows Z: RiskParity and
    HierarchicalRiskParity solve on that k-row window form, the QP objectives on the dense
    estimate (``estimate_batch_lr`` does not serve 'pca').

    method 'gerber' (spec ``threshold`` in (0, 1], default 0.5, and ``variant`` 1 or 2, default 2;
    anything else raises ValueError before the device is touched): the dense estimate of
    engine.gerber_cov.  Its thresholds are the window's own standard deviations, so there is no
    window form shared between dates: ``estimate_batch_lr`` serves it with ``materialise=True``
    only.  Variant 2 is positive semi-definite by construction, variant 1 can be indefinite.

    methods 'spearman' and 'kendall' (no parameters): the dense estimate of engine.rank_cov, for
    complete windows.  Both are positive semi-definite by construction, and Kendall's tau-b is
    positive definite on typical windows with more assets than rows, where Spearman's rho (like the
    sample covariance) is singular.  The ranks belong to each date's own window, so
    ``estimate_batch_lr`` serves them with ``materialise=True`` only.

    method 'ewma' (spec ``halflife`` in rows, > 0, inf allowed, or ``decay`` in (0, 1]; both raise
    ValueError, neither means decay = 0.94, the RiskMetrics daily value; a bad value raises
    ValueError before the device is touched): the dense estimate of engine.ewma_cov, for complete
    windows, positive semi-definite by construction.  The weight of a row depends on its age in
    each date's window, so ``estimate_batch_lr`` serves it with ``materialise=True`` only; with a
    ``plan`` the dates of a slide group are formed by the decaying recursion."""

    def __init__(self, spec: CovarianceSpecification = None, *args, **kwargs):
        self.spec = CovarianceSpecification(*args, **kwargs) if spec is None else spec
        if self.spec["method"] == "gerber":
            self.gerber_spec   # a bad threshold or variant is refused here, before any device work
        if self.spec["method"] == "ewma":
            self.ewma_spec     # likewise a bad halflife or decay
        self.shrinkage_ = None
        self.shrinkage_batch_ = None
        self.n_factors_ = None
        self.noise_variance_ = None
        self.n_factors_batch_ = None
        self.noise_variance_batch_ = None

    def set_ctrl(self, *args, **kwargs) -> None:
        self.spec = CovarianceSpecification(*args, **kwargs)

    def estimate(self, X: pd.DataFrame):
        method = self.spec["method"]
        if method == "pearson":
            covmat = cov_pearson(X)
        elif method == "duv":
            covmat = cov_duv(X)
        elif method == "linear_shrinkage":
            covmat = cov_linear_shrinkage(X, self.spec.get("lambda_covmat_regularization"))
        elif method in SHRINKAGE_METHODS:
            covmat, self.shrinkage_ = _cov_shrunk(X, method)
        elif method == "pca":
            covmat, self.n_factors_, self.noise_variance_ = _cov_pca(X, self.n_factors)
        elif method == "gerber":
            covmat = cov_gerber(X, *self.gerber_spec)
        elif method in RANK_METHODS:
            covmat = _cov_rank(X, method)
        elif method == "ewma":
            covmat = cov_ewma(X, *self.ewma_spec)
        else:
            raise NotImplementedError("This method is not implemented yet")
        if self.spec.get("check_positive_definite") and not isPD(covmat):
            fixed = nearestPD(covmat)
            covmat = pd.DataFrame(fixed, index=covmat.index, columns=covmat.columns) \
                if isinstance(covmat, pd.DataFrame) else fixed
        return covmat

    @property
    def n_factors(self):
        """The spec's ``n_factors`` of method 'pca' ('mp' where none is given)."""
        nf = self.spec.get("n_factors")
        return "mp" if nf is None else nf

    @property
    def gerber_spec(self):
        """(threshold, variant) of method 'gerber' (0.5 and 2 where the spec gives none);
        ValueError for a threshold outside (0, 1] or a variant other than 1 or 2."""
        th, var = self.spec.get("threshold"), self.spec.get("variant")
        return _gerber_check(0.5 if th is None else th, 2 if var is None else var)

    @property
    def ewma_spec(self):
        """(halflife, decay) of method 'ewma', one of them None (decay 0.94 where the spec gives
        neither); ValueError for both given or a value outside its range."""
        return _ewma_check(self.spec.get("halflife"), self.spec.get("decay"))

    def window_form_pca(self, panel, rows, tlen):
        """method 'pca' for every window of the device row table: engine.pca_window_form's factor
        form (Sigma_b = Z_b'Z_b + sigma2[b] I), the per-date factor counts and noise levels kept
        in ``n_factors_batch_`` / ``noise_variance_batch_``."""
        from . import engine
        form = engine.pca_window_form(panel, rows, tlen, n_factors=self.n_factors)
        self.n_factors_batch_, self.noise_variance_batch_ = form.tlen, form.sigma2
        return form

    def _estimate_batch_pairwise(self, panel, rows, tlen, out, method):
        r = _pairwise_batch(panel, rows, tlen, out, method, self.spec.get("lambda_covmat_regularization"),
                            bool(self.spec.get("check_positive_definite")))
        return (None, None, None, None) if r is None else r

    # -- batched (backtest) entry --------------------------------------------------------
    def estimate_batch(self, panel, rows, tlen, out=None, plan=None, lower_only=False):
        """All dates at once on the device.  Returns (S, p_diag): S is the (B, ld, ld)
        device tensor of raw sample covariances; p_diag (B,) is the diagonal term the spec
        adds (linear shrinkage: lam * mean(diag S)); 'duv' returns (None, None)."""
        S, pdiag, _, _ = self.estimate_batch_lr(panel, rows, tlen, out=out, plan=plan, lower_only=lower_only)
        return S, pdiag

    def estimate_batch_lr(self, panel, rows, tlen, out=None, plan=None, lower_only=False,
                          materialise=True, groups=None):
        """estimate_batch plus the window means (the centring of the factored form
        S = Xc'Xc / (T-1) that the low-rank solver uses) -> (S, p_diag, mu, dg).
        ``plan``: an engine.SlidePlan for overlapping windows; ``lower_only``: lower-triangle
        storage.  ``materialise=False`` (the window-form solver, which never reads an n x n
        S): S is None and dg = diag(Xc'Xc) per date carries what the shrinkage term needs."""
        import torch
        method = self.spec["method"]
        self.shrinkage_batch_ = None
        if method == "duv":
            return None, None, None, None
        if method == "pca":
            raise NotImplementedError("the 'pca' covariance is not a T-row window form: window_form_pca gives its "
                                      "factor form, estimate the dense matrix")
        if method == "gerber":
            threshold, variant = self.gerber_spec
            if not materialise:
                raise NotImplementedError("the 'gerber' covariance has no window form: its thresholds are the "
                                          "standard deviations of each date's own window, so no rows are shared "
                                          "between dates; estimate the dense matrix (materialise=True)")
            if panel.has_nan:   # complete windows only: the serial loop reports it
                return None, None, None, None
            from . import engine
            n = panel.n
            if out is not None:   # the kernel writes [0, n) x [0, n) only: the padding of a dense P is zero
                out[:, n:, :] = 0.0
                out[:, :n, n:] = 0.0
            S, _, _ = engine.gerber_cov(panel, rows, tlen, threshold=threshold, variant=variant, out=out)
            return S, torch.zeros(int(rows.shape[0]), dtype=torch.float64, device=S.device), None, None
        if method in RANK_METHODS:
            if not materialise:
                raise NotImplementedError(f"the {method!r} covariance has no window form: the ranks belong to each "
                                          "date's own window, so no rows are shared between dates; estimate the "
                                          "dense matrix (materialise=True)")
            if panel.has_nan:   # complete windows only: the serial loop reports it
                return None, None, None, None
            from . import engine
            S, _, _ = engine.rank_cov(panel, rows, tlen, kind=method, out=out)   # (it zeroes the padding)
            return S, torch.zeros(int(rows.shape[0]), dtype=torch.float64, device=S.device), None, None
        if method == "ewma":
            halflife, decay = self.ewma_spec
            if not materialise:
                raise NotImplementedError("the 'ewma' covariance has no window form: the weight of a row is "
                                          "its age in each date's own window and so differs from date to date, "
                                          "the dates of a slide group share no scaled row; estimate the dense "
                                          "matrix (materialise=True)")
            if panel.has_nan:   # complete windows only: the serial loop reports it
                return None, None, None, None
            from . import engine
            S, _, _ = engine.ewma_cov(panel, rows, tlen, halflife=halflife, decay=decay, plan=plan,
                                      out=out)   # (it zeroes the padding)
            return S, torch.zeros(int(rows.shape[0]), dtype=torch.float64, device=S.device), None, None
        if method not in ("pearson", "linear_shrinkage") + SHRINKAGE_METHODS:
            raise NotImplementedError("This method is not implemented yet")
        B, n = int(rows.shape[0]), panel.n
        if panel.has_nan:
            if method in SHRINKAGE_METHODS:   # complete windows only: the serial loop reports it
                return None, None, None, None
            return self._estimate_batch_pairwise(panel, rows, tlen, out, method)
        S = dg = None
        if not materialise and groups is not None and groups.ok:
            # the window form with slide groups (engine.GroupPlan): means and diag(Xc'Xc) of
            # every window in one sliding pass per group instead of two passes per window
            ld = ((n + 63) // 64) * 64
            mu = torch.zeros((B, ld), dtype=torch.float64, device=panel.device)
            dg = torch.zeros((B, ld), dtype=torch.float64, device=panel.device)
            panel.window_moments_grouped(groups, tlen, mu, dg)
        else:
            mu = panel.window_means(rows, tlen)
            if materialise:
                S = panel.cov(rows, tlen, mode=0, out=out, mu=mu, plan=plan,
                              lower_only=lower_only and plan is not None)
            else:
                dg = panel.window_sumsq(rows, tlen, mu)
        pdiag = torch.zeros(B, dtype=torch.float64, device=mu.device)
        if method == "linear_shrinkage":
            lam = _shrink_lambda(self.spec.get("lambda_covmat_regularization"))
            if lam > 0:
                if S is not None:
                    pdiag = lam * torch.diagonal(S, dim1=1, dim2=2)[:, :n].mean(dim=1)
                else:   # mean(diag S) = mean(diag Xc'Xc) / (T - 1)
                    pdiag = lam * dg[:, :n].mean(dim=1) / (tlen.to(torch.float64) - 1.0)
        elif method in SHRINKAGE_METHODS:
            from . import engine
            delta, _ = engine.shrinkage_intensity(panel, rows, tlen, kind=method)
            self.shrinkage_batch_ = delta
            if S is not None:
                pdiag = delta * torch.diagonal(S, dim1=1, dim2=2)[:, :n].mean(dim=1)
            else:
                pdiag = delta * dg[:, :n].mean(dim=1) / (tlen.to(torch.float64) - 1.0)
        return S, pdiag, mu, dg


def _pairwise_batch(panel, rows, tlen, out, method, lam_raw, check_pd):
    """Windows with missing values, all dates at once: pairwise-complete covariance
    (pq_cov_pairwise_batched), the linear-shrinkage term, then Covariance.estimate's PD check
    and nearestPD repair for the dates that need it (src/covariance.py:50-54) -> (S, 0, None,
    None); None when some pair has fewer than 2 common rows (the reference fails there too)."""
    import torch
    from .helper_functions import nearestPD_device, pd_info_device
    S = panel.cov_pairwise(rows, tlen, out=out)
    n = panel.n
    if bool(torch.isnan(S[:, :n, :n]).any().item()):
        return None
    B = S.shape[0]
    idx = torch.arange(n, device=S.device)
    if method == "linear_shrinkage":
        lam = _shrink_lambda(lam_raw)
        if lam > 0:
            md = torch.diagonal(S, dim1=1, dim2=2)[:, :n].mean(dim=1)
            S[:, idx, idx] += (lam * md)[:, None]
    if check_pd:   # on the device: K2 info for every date, the repair for the failing ones only
        bad = torch.nonzero(pd_info_device(S, n) != 0).flatten()
        if bad.numel():
            S[bad, :n, :n] = nearestPD_device(S[bad], n)[:, :n, :n]
    return S, torch.zeros(B, dtype=torch.float64, device=S.device), None, None


def _device_cov(X, mode=0):
    from . import engine
    Xv = np.ascontiguousarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
    T, n = Xv.shape
    pan = engine.Panel(Xv)
    rows, tlen = pan.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
    if mode == 0 and np.isnan(Xv).any():
        # missing values: pandas' pairwise-complete DataFrame.cov() (pq_cov_pairwise_batched)
        S = pan.cov_pairwise(rows, tlen)
    else:
        S = pan.cov(rows, tlen, mode=mode)
    return S[0, :n, :n].cpu().numpy()


def cov_pearson(X):
    """X.cov() (src/covariance.py:65-66) on the device."""
    S = _device_cov(X, mode=0)
    if isinstance(X, pd.DataFrame):
        return pd.DataFrame(S, index=X.columns, columns=X.columns)
    return S


def cov_duv(X):
    """Identity, returned as an ndarray like the reference (src/covariance.py:68-69)."""
    return np.identity(X.shape[1])


def cov_linear_shrinkage(X, lambda_covmat_regularization=None):
    """Sigma + lambda * mean(diag Sigma) * I (src/covariance.py:71-84); the reference's
    unused correlation loop (:78-82) is not reproduced (it has no effect on the result)."""
    lam = _shrink_lambda(lambda_covmat_regularization)
    S = cov_pearson(X)
    if lam > 0:
        vals = S.to_numpy() if isinstance(S, pd.DataFrame) else S
        d = vals.shape[0]
        vals = vals + lam * np.mean(np.diag(vals)) * np.eye(d)
        S = pd.DataFrame(vals, index=S.index, columns=S.columns) if isinstance(S, pd.DataFrame) else vals
    return S


def _cov_shrunk(X, method):
    """(Sigma*, delta) of one complete window: the sample covariance (K1) shrunk towards
    mean(diag S) I by the intensity of engine.shrinkage_intensity."""
    from . import engine
    Xv = np.ascontiguousarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
    if np.isnan(Xv).any():
        raise ValueError(f"{method} shrinkage needs complete windows")
    T, n = Xv.shape
    pan = engine.Panel(Xv)
    rows, tlen = pan.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
    S = pan.cov(rows, tlen, mode=0)[0, :n, :n].cpu().numpy()
    delta = float(engine.shrinkage_intensity(pan, rows, tlen, kind=method)[0][0].item())
    S = (1.0 - delta) * S + delta * np.mean(np.diag(S)) * np.eye(n)
    if isinstance(X, pd.DataFrame):
        S = pd.DataFrame(S, index=X.columns, columns=X.columns)
    return S, delta


def _cov_pca(X, n_factors="mp"):
    """(Sigma, k, sigma2) of one complete window: the dense Z'Z + sigma2 I of
    engine.pca_window_form at batch 1."""
    from . import _lib, engine
    Xv = np.ascontiguousarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
    if np.isnan(Xv).any():
        raise ValueError("the pca covariance needs complete windows")
    T, n = Xv.shape
    pan = engine.Panel(Xv)
    rows, tlen = pan.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
    form = engine.pca_window_form(pan, rows, tlen, n_factors=n_factors)
    if int(form.status[0].item()) != _lib.PQ_PCA_OK:
        raise ValueError("the pca covariance: bad input (fewer than 2 rows, non-finite data, more factors than "
                         "the window has rank, or no variance left for the noise level)")
    S = form.dense(0).cpu().numpy()
    if isinstance(X, pd.DataFrame):
        S = pd.DataFrame(S, index=X.columns, columns=X.columns)
    return S, int(form.tlen[0].item()), float(form.sigma2[0].item())


def _gerber_check(threshold, variant):
    """(threshold, variant) as (float, int); ValueError unless 0 < threshold <= 1 and variant is 1 or 2
    (host arithmetic only: a spec is refused before anything touches the device)."""
    if isinstance(variant, bool) or not isinstance(variant, (int, np.integer)) or variant not in (1, 2):
        raise ValueError(f"gerber: variant = {variant!r} must be 1 or 2")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
            or not 0.0 < float(threshold) <= 1.0:
        raise ValueError(f"gerber: threshold = {threshold!r} must lie in (0, 1]")
    return float(threshold), int(variant)


def cov_gerber(X, threshold=0.5, variant=2):
    """Gerber covariance (Gerber et al. 2022) of one complete window: engine.gerber_cov at batch
    1.  ``threshold`` in (0, 1]: the multiple of an asset's window standard deviation beyond
    which a day counts as a move; ``variant`` 2 (positive semi-definite) or 1 (the paper's first
    form).  ValueError for a bad spec, missing values or a bad-input window."""
    threshold, variant = _gerber_check(threshold, variant)
    from . import _lib, engine
    Xv = np.ascontiguousarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
    if np.isnan(Xv).any():
        raise ValueError("the gerber covariance needs complete windows")
    T, n = Xv.shape
    pan = engine.Panel(Xv)
    rows, tlen = pan.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
    S, status, _ = engine.gerber_cov(pan, rows, tlen, threshold=threshold, variant=variant)
    if int(status[0].item()) != _lib.PQ_GERBER_OK:
        raise ValueError("the gerber covariance: bad input (fewer than 2 rows, non-finite data, a constant column, "
                         "or an asset that never moves beyond its threshold)")
    S = S[0, :n, :n].cpu().numpy()
    if isinstance(X, pd.DataFrame):
        S = pd.DataFrame(S, index=X.columns, columns=X.columns)
    return S


def _cov_rank(X, kind):
    """engine.rank_cov at batch 1 on one complete window; ValueError for missing values or bad input."""
    from . import _lib, engine
    Xv = np.ascontiguousarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
    if np.isnan(Xv).any():
        raise ValueError(f"the {kind} covariance needs complete windows")
    T, n = Xv.shape
    if not 1 <= T <= _lib.PQ_RANK_TMAX:
        raise ValueError(f"the {kind} covariance: bad input ({T} rows, supported: 2..{_lib.PQ_RANK_TMAX})")
    pan = engine.Panel(Xv)
    rows, tlen = pan.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
    S, status, _ = engine.rank_cov(pan, rows, tlen, kind=kind)
    if int(status[0].item()) != _lib.PQ_RANK_OK:
        raise ValueError(f"the {kind} covariance: bad input (fewer than 2 rows, non-finite data or a constant column)")
    S = S[0, :n, :n].cpu().numpy()
    if isinstance(X, pd.DataFrame):
        S = pd.DataFrame(S, index=X.columns, columns=X.columns)
    return S


EWMA_DEFAULT_DECAY = 0.94   # RiskMetrics' daily value


def _ewma_check(halflife, decay):
    """(halflife, decay) as floats, one of them None; neither given: decay = EWMA_DEFAULT_DECAY.
    ValueError for both given, a halflife not > 0 (inf is allowed, NaN is not) or a decay outside
    (0, 1] (host arithmetic only: a spec is refused before anything touches the device)."""
    def real(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))
    if halflife is not None and decay is not None:
        raise ValueError("ewma: give halflife or decay, not both")
    if halflife is not None:
        if not real(halflife) or not float(halflife) > 0.0:
            raise ValueError(f"ewma: halflife = {halflife!r} must be > 0 (rows; inf allowed)")
        return float(halflife), None
    if decay is None:
        return None, EWMA_DEFAULT_DECAY
    if not real(decay) or not 0.0 < float(decay) <= 1.0:
        raise ValueError(f"ewma: decay = {decay!r} must lie in (0, 1]")
    return None, float(decay)


def cov_ewma(X, halflife=None, decay=None):
    """Exponentially weighted covariance (RiskMetrics 1996) of one complete window, oldest row
    first: engine.ewma_cov at batch 1 -- np.cov(X, rowvar=False, aweights=w) with
    w = 0.5 ** (age / halflife) or decay ** age, the last block of
    X.ewm(halflife=h).cov(bias=False).  ValueError for a bad spec, missing values or a bad-input
    window."""
    halflife, decay = _ewma_check(halflife, decay)
    from . import _lib, engine
    Xv = np.ascontiguousarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
    if np.isnan(Xv).any():
        raise ValueError("the ewma covariance needs complete windows")
    T, n = Xv.shape
    if not 1 <= T <= _lib.PQ_EWMA_TMAX:
        raise ValueError(f"the ewma covariance: bad input ({T} rows, supported: 2..{_lib.PQ_EWMA_TMAX})")
    pan = engine.Panel(Xv)
    rows, tlen = pan.rows_to_device(np.arange(T, dtype=np.int32)[None], np.array([T], dtype=np.int32))
    S, status, _ = engine.ewma_cov(pan, rows, tlen, halflife=halflife, decay=decay)
    if int(status[0].item()) != _lib.PQ_EWMA_OK:
        raise ValueError("the ewma covariance: bad input (fewer than 2 rows, non-finite data, or a decay so fast "
                         "that only the newest row has weight)")
    S = S[0, :n, :n].cpu().numpy()
    if isinstance(X, pd.DataFrame):
        S = pd.DataFrame(S, index=X.columns, columns=X.columns)
    return S


def cov_spearman(X):
    """Spearman rank covariance of one complete window: Spearman's rho of the columns (mid-ranks
    for ties) times the outer product of the window's standard deviations.  Positive
    semi-definite.  ValueError for missing values or a bad-input window."""
    return _cov_rank(X, "spearman")


def cov_kendall(X):
    """Kendall rank covariance of one complete window: Kendall's tau-b of the columns times the
    outer product of the window's standard deviations.  Positive semi-definite, and positive
    definite on typical windows with more assets than rows.  ValueError for missing values or a
    bad-input window."""
    return _cov_rank(X, "kendall")


def cov_ledoit_wolf(X):
    """Ledoit-Wolf (2004) shrinkage of the sample covariance towards mean(diag S) I with the
    intensity of sklearn's ledoit_wolf_shrinkage (applied to the ddof = 1 covariance)."""
    return _cov_shrunk(X, "ledoit_wolf")[0]


def cov_oas(X):
    """Oracle approximating shrinkage (Chen et al. 2010), sklearn's oas intensity."""
    return _cov_shrunk(X, "oas")[0]


def cov_pca(X, n_factors="mp"):
    """PCA factor covariance (probabilistic PCA, sklearn's PCA.get_covariance() with the noise
    level averaged over n - k): the top ``n_factors`` principal components, 'mp': the
    Marchenko-Pastur count (engine.pca_window_form)."""
    return _cov_pca(X, n_factors)[0]
