"""Host side of the quantile portfolios (no device): the numpy yardstick against the
reference fixture, the host index plan + two-branch lerp against np.percentile bit for bit,
and the output_to_strategies helper."""
import os

import numpy as np
import pandas as pd
import pytest

from porqua_amd import engine
from porqua_amd.helper_functions import output_to_strategies
from porqua_amd.portfolio import Strategy

from tests.percentile_model import batch_model, lerp_thresholds, reference_solve

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msci_percentile.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("N", [1, 3, 5])
def test_restatement_reproduces_the_reference_fixture(N):
    g = np.load(GOLDEN)
    assert float(g["min_gap"]) >= 1e-9 and int(g["b_dropped"]) <= 0.05 * len(g["b_all_rebdates"])
    for s, th, w, masks in zip(g["a_scores"], g[f"a_th_{N}"], g[f"a_w_{N}"], g[f"a_masks_{N}"]):
        th_m, masks_m, w_m = reference_solve(-s, N)
        assert np.array_equal(_bits(th_m), _bits(th))
        assert np.array_equal(np.array(masks_m), masks)
        assert np.array_equal(w_m, w)
        bt = batch_model(s[None], N)
        assert np.array_equal(bt[3][0], w) and bt[4][0] == 0
        assert all(np.array_equal(bt[1][0] == i + 1, masks[i]) for i in range(N))
    if N == 5:   # the walkthrough's backtest dates
        for s, w, masks in zip(g["b_scores"], g["b_w"], g["b_masks"]):
            _, masks_m, w_m = reference_solve(-s, N)
            assert np.array_equal(np.array(masks_m), masks) and np.array_equal(w_m, w)


def _rows(n, rng):
    """Continuous, tie-heavy (one decimal) and integer-valued (with both zeros) rows."""
    a = rng.standard_normal(n)
    b = np.round(rng.standard_normal(n), 1)
    c = rng.integers(-3, 4, n).astype(np.float64)
    c[c == 0] *= rng.choice([-1.0, 1.0], int((c == 0).sum()))
    return a, b, c


def test_host_plan_and_lerp_equal_np_percentile_bitwise():
    rng = np.random.default_rng(20240607)
    sizes = list(range(1, 301)) + [494, 1000, 1001, 4097, 16384]
    for n in sizes:
        rows = [(x, np.sort(x)) for x in _rows(n, rng)]
        for N in (1, 2, 3, 5, 10):
            prev, nxt, gamma = engine.percentile_plan(n, N)
            assert prev.dtype == np.int32 and gamma.dtype == np.float64 and len(prev) == N + 1
            assert prev.min() >= 0 and max(prev.max(), nxt.max()) <= n - 1
            for x, xs in rows:
                ref = np.percentile(x, np.linspace(0, 100, N + 1))
                got = lerp_thresholds(xs, prev, nxt, gamma)
                # equal values everywhere; equal bits too wherever the value is not a zero (which
                # of -0.0 / +0.0 sits at an order statistic is the sorter's choice, in numpy too)
                assert np.array_equal(got, ref), (n, N)
                nz = ref != 0
                assert np.array_equal(_bits(got)[nz], _bits(ref)[nz]), (n, N)


def test_output_to_strategies():
    idx = ["A", "B", "C", "D"]
    output = {
        "2020-01-31": {"weights_1": pd.Series({"A": 0.5, "B": 0.5}), "weights_2": pd.Series({"C": 0.5, "D": 0.5})},
        "2020-02-28": {"weights_1": pd.Series({"C": 1.0}), "weights_2": {"A": 1 / 3, "B": 1 / 3, "D": 1 / 3}},
    }
    sd = output_to_strategies(output)
    assert list(sd) == ["q1", "q2"] and all(isinstance(s, Strategy) for s in sd.values())
    assert [p.rebalancing_date for p in sd["q1"].portfolios] == ["2020-01-31", "2020-02-28"]
    assert sd["q1"].portfolios[0].weights == {"A": 0.5, "B": 0.5}
    assert sd["q1"].portfolios[1].weights == {"C": 1.0}
    assert sd["q2"].portfolios[0].weights == {"C": 0.5, "D": 0.5}
    assert sd["q2"].portfolios[1].weights == {"A": 1 / 3, "B": 1 / 3, "D": 1 / 3}
    assert set(idx) >= set().union(*(p.weights for s in sd.values() for p in s.portfolios))
