"""Write tests/golden/trend_cases.npz: small block-statistic series with the trends marineHeatWaves.meanTrend's
formula and the textbook Theil-Sen / Mann-Kendall definitions give them, computed here by independent routes
(numpy.linalg.lstsq as meanTrend does; numpy.median of the pairwise slopes; a Python loop for S and the tie
groups) -- not by the oracle of the tests.

    python tools/make_golden_trend.py
"""
import itertools
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "trend_cases.npz")


def cases():
    rng = np.random.default_rng(2024)
    nb = 21
    years = np.arange(1982, 1982 + nb)
    y = np.empty((nb, 12))
    y[:, 0] = rng.poisson(2.0, nb)                                   # ecount: ties
    y[:, 1] = rng.poisson(2.0, nb) + np.arange(nb) // 5              # ecount with a trend
    y[:, 2] = 10 + 0.3 * np.arange(nb) + rng.normal(size=nb)         # duration
    y[:, 3] = rng.normal(size=nb)
    y[:, 4] = 3.0                                                    # all equal
    y[:, 5] = np.arange(nb) * 0.5 - 3                                # strictly increasing
    y[:, 6] = -np.arange(nb) ** 2                                    # strictly decreasing
    y[:, 7] = rng.integers(0, 4, nb)
    y[:, 8] = rng.normal(size=nb) * 1e-3 + 2
    y[:, 9] = rng.integers(0, 30, nb)                                # day counts
    y[:, 10] = rng.normal(size=nb)
    y[:, 11] = rng.poisson(1.0, nb)
    y[rng.random(nb) < 0.3, 3] = np.nan
    y[::2, 8] = np.nan
    y[[0, 5, 20], 9] = np.nan
    y[3:, 10] = np.nan                                               # three valid blocks
    return years, y


def expected(years, y):
    x = years - years.mean()
    C = y.shape[1]
    ols = np.full((2, C), np.nan)
    ts = np.full((3, C), np.nan)
    for c in range(C):
        v = ~np.isnan(y[:, c])
        xx, yy = x[v], y[v, c]
        beta = np.linalg.lstsq(np.stack([np.ones(xx.size), xx], axis=1), yy, rcond=None)[0]     # meanTrend's route
        ols[:, c] = beta
        pairs = list(itertools.combinations(range(xx.size), 2))
        ts[0, c] = np.median([(yy[j] - yy[i]) / (xx[j] - xx[i]) for i, j in pairs])
        ts[1, c] = sum(int(np.sign(yy[j] - yy[i])) for i, j in pairs)
        m = xx.size
        groups = np.unique(yy, return_counts=True)[1]
        ts[2, c] = (m * (m - 1) * (2 * m + 5) - sum(int(t) * (t - 1) * (2 * t + 5) for t in groups)) / 18
    return ols, ts


if __name__ == "__main__":
    years, y = cases()
    ols, ts = expected(years, y)
    np.savez(OUT, years=years, y=y, ols_mean_trend=ols, ts_trend_s_var=ts)
    print("wrote", os.path.normpath(OUT), os.path.getsize(OUT), "bytes")
