"""Numpy yardstick of the quantile-portfolio kernel: PercentilePortfolios.solve
(src/optimization.py:398-417) restated line for line on arrays.

``reference_solve`` takes the objective's score vector (the reference's ``-scores``) and
returns what the reference builds from it, raising ZeroDivisionError where the reference does.
``batch_model`` applies it to every row of a raw score panel and lays the answers out as
pq_percentile_batched does, failing rows included (include/porqua_hip.h)."""
import numpy as np

PCT_OK, PCT_EMPTY_BUCKET, PCT_NAN_SCORE = 0, 1, 2


def reference_solve(scores: np.ndarray, N: int):
    """(th, masks, weights): thresholds, one member mask per bucket and the long-short weights
    of one score vector; 1 / len(bucket) raises ZeroDivisionError on an empty bucket."""
    q_vec = np.linspace(0, 100, N + 1)
    th = np.percentile(scores, q_vec)
    masks = []
    w_val = {}
    for i in range(1, len(th)):
        if i == 1:
            masks.append(scores <= th[i])
        else:
            masks.append(np.logical_and(scores > th[i - 1], scores <= th[i]))
        w_val[i] = 1 / int(masks[i - 1].sum())
    weights = scores * 0
    weights[masks[0]] = 1 / int(masks[0].sum())
    weights[masks[N - 1]] = -1 / int(masks[N - 1].sum())
    return th, masks, weights


def lerp_thresholds(sorted_x: np.ndarray, prev, nxt, gamma) -> np.ndarray:
    """The kernel's thresholds from a sorted row and the host plan: numpy's two-branch _lerp,
    each operation rounded on its own (no fused multiply-add)."""
    a, b = sorted_x[prev], sorted_x[nxt]
    d = b - a
    out = a + d * gamma
    hi = gamma >= 0.5
    out[hi] = (b - d * (1 - gamma))[hi]
    return out


def batch_model(X: np.ndarray, N: int, sign: float = -1.0):
    """(th [B, N+1], bucket [B, n], counts [B, N], w [B, n], status [B]) of the raw score panel
    X as the kernel lays them out: a row with a NaN has NaN th and w and zero bucket / counts;
    a row with an empty bucket keeps th, bucket and counts and has NaN w."""
    B, n = X.shape
    th = np.full((B, N + 1), np.nan)
    bucket = np.zeros((B, n), dtype=np.int32)
    counts = np.zeros((B, N), dtype=np.int32)
    w = np.full((B, n), np.nan)
    status = np.zeros(B, dtype=np.int32)
    for r in range(B):
        x = sign * X[r]
        if np.isnan(x).any():
            status[r] = PCT_NAN_SCORE
            continue
        th[r] = np.percentile(x, np.linspace(0, 100, N + 1))
        for i in range(1, N + 1):
            m = x <= th[r, 1] if i == 1 else np.logical_and(x > th[r, i - 1], x <= th[r, i])
            assert not bucket[r][m].any()          # the reference's masks are disjoint
            bucket[r][m] = i
            counts[r, i - 1] = m.sum()
        assert counts[r].sum() == n                # ... and cover the universe
        try:
            w[r] = reference_solve(x, N)[2]
        except ZeroDivisionError:
            assert counts[r].min() == 0
            status[r] = PCT_EMPTY_BUCKET
        else:
            assert counts[r].min() > 0
    return th, bucket, counts, w, status
