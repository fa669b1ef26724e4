"""The longdouble model of the exponentially weighted covariance (tests/ewma_model.py) against
NumPy's np.cov(aweights=) and pandas' ewm().cov(), the age table of both parameterisations and the
spec validation -- host only."""
import numpy as np
import pandas as pd
import pytest

from porqua_amd.covariance import Covariance, _ewma_check
from porqua_amd.engine import ewma_age_weights
from tests import ewma_model as em

# np.cov and pandas sum T <= 60 float64 products per entry; both were seen to agree with the longdouble
# model to 4e-16 of the largest variance.  A few ulps (2^-52 = 2.2e-16 each) of the largest variance:
ULPS = 8 * 2.0 ** -52


def _windows():
    rng = np.random.default_rng(11)
    for T, n in [(2, 3), (17, 5), (40, 12), (60, 7)]:
        yield 0.01 * rng.standard_normal((T, n)) + 0.001 * rng.standard_normal(n)


def test_model_is_numpy_and_pandas():
    h = 11.0
    for X in _windows():
        T = X.shape[0]
        wage = ewma_age_weights(T, halflife=h)
        mod = em.ewma(X, wage)
        assert mod.status == em.OK
        S = mod.Sigma.astype(np.float64)
        bar = ULPS * float(np.diag(S).max())
        ref = np.cov(X, rowvar=False, aweights=wage[:T][::-1])
        assert np.abs(S - ref).max() <= bar
        last = pd.DataFrame(X).ewm(halflife=h, adjust=True).cov(bias=False).to_numpy()[-X.shape[1]:]
        assert np.abs(S - last).max() <= bar
        mp = pd.DataFrame(X).ewm(halflife=h, adjust=True).mean().to_numpy()[-1]
        assert np.abs(mod.mean.astype(np.float64) - mp).max() <= ULPS * np.abs(X).max()
        assert np.linalg.eigvalsh(S).min() >= -bar * X.shape[1]      # PSD up to rounding


def test_infinite_halflife_is_the_sample_covariance():
    for X in _windows():
        T = X.shape[0]
        for wage in (ewma_age_weights(T, halflife=np.inf), ewma_age_weights(T, decay=1.0)):
            assert np.array_equal(wage, np.ones(T + 1))
            mod = em.ewma(X, wage)
            assert float(mod.den) == T - 1
            S = mod.Sigma.astype(np.float64)
            assert np.abs(S - np.cov(X, rowvar=False)).max() <= ULPS * float(np.diag(S).max())


def test_age_table():
    k = np.arange(301, dtype=np.float64)
    assert np.array_equal(ewma_age_weights(300, halflife=11.2), 0.5 ** (k / 11.2))
    assert np.array_equal(ewma_age_weights(300, decay=0.97), 0.97 ** k)
    assert np.array_equal(ewma_age_weights(300), 0.94 ** k)          # neither: RiskMetrics' daily value
    w = ewma_age_weights(64, halflife=8)
    assert w[0] == 1.0 and w[8] == 0.5 and w[64] == 2.0 ** -8 and len(w) == 65
    assert w.dtype == np.float64 and np.all(np.diff(w) < 0)
    # the two parameterisations name the same weights: decay = 0.5 ** (1 / halflife)
    np.testing.assert_allclose(ewma_age_weights(64, decay=0.5 ** (1 / 8)), w, rtol=1e-14)


def test_bad_windows():
    X = next(iter(_windows()))
    wage = ewma_age_weights(40, halflife=11)
    assert em.ewma(X[:1], wage).status == em.BAD_INPUT
    for v in (np.nan, np.inf):
        Y = np.vstack([X, X])
        Y[1, 1] = v
        assert em.ewma(Y, wage).status == em.BAD_INPUT
    # a half-life so small that only the newest row has weight in float64: W1 = W2 = 1
    assert em.ewma(np.vstack([X, X]), ewma_age_weights(40, halflife=0.01)).status == em.BAD_INPUT


@pytest.mark.parametrize("kw", [{"halflife": 5, "decay": 0.9}, {"decay": 0}, {"decay": 1.5}, {"decay": -0.1},
                                {"halflife": 0}, {"halflife": -3.0}, {"halflife": True}, {"decay": True},
                                {"halflife": float("nan")}, {"decay": float("nan")}, {"halflife": "11"}])
def test_spec_validation(kw):
    with pytest.raises(ValueError, match="ewma"):
        _ewma_check(kw.get("halflife"), kw.get("decay"))
    with pytest.raises(ValueError, match="ewma"):
        Covariance(method="ewma", **kw)
    with pytest.raises(ValueError, match="ewma"):
        ewma_age_weights(10, **kw)


def test_spec_defaults():
    assert _ewma_check(None, None) == (None, 0.94)
    assert _ewma_check(np.inf, None) == (np.inf, None)
    assert _ewma_check(None, 1) == (None, 1.0)
    assert Covariance(method="ewma").ewma_spec == (None, 0.94)
    assert Covariance(method="ewma", halflife=21).ewma_spec == (21.0, None)
