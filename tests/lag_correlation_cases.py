"""The case generators shared by the host and the GPU tests of lag_correlation(): two series around their bases with the
columns that can go wrong made by construction, and class patterns.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

# L: L + 1 = 1, 8, 9, 16, 17, 33, 48, 49, 64 -- every ring depth (16, 32, 64 slots) and every lag group edge (one group of
# 8 up to 8 lags, groups of 16 beyond)
DEPTH_LAGS = (0, 7, 8, 15, 16, 32, 47, 48, 63)
LONG_RUN = 70                                   # a run of NaN longer than the largest lag


def series(T, C, dtype, seed, Dr=1):
    """x and y (T, C) around base_x and base_y (Dr, C): persistent anomalies of a few units (so that lagged products do
    not cancel), y = a lagged mix of x and noise, zeros among them, 3 % scattered NaN, and by column (where C and T allow)
      2  y all NaN            3  x all NaN
      4  a run of LONG_RUN NaN in y from step 20        5  the same in x from step 90
      6  a few out-of-range values in x and in y, infinities among them
      7  x exactly at base + 128 at one step and base - 128 at another; y one unit of the fixed point inside
    With Dr > 1 row_of_t is not monotone.  Returns x, y, base_x, base_y, rows, doy, doys."""
    rng = np.random.default_rng(seed)
    bx = np.round(18.0 + 6.0 * rng.random((Dr, C)), 2)
    by = np.round(-3.0 + 2.0 * rng.random((Dr, C)), 2)
    doys = np.arange(1, Dr + 1) if Dr > 1 else np.zeros(1, dtype=np.int64)
    rows = ((np.arange(T) * 3 + 2) % Dr).astype(np.int32)
    e = rng.normal(0, 1.0, (T, C))
    a = np.zeros((T, C))
    for t in range(T):
        a[t] = (0.8 * a[t - 1] if t else 0.0) + e[t]
    a = np.round(a + 0.5, 3)
    b = np.round(0.6 * np.roll(a, 3, axis=0) + rng.normal(0, 1.0, (T, C)) - 0.25, 3)
    for v in (a, b):
        v[rng.random((T, C)) < 0.03] = 0.0
    if C > 7:
        bx[:, 7], by[:, 7] = 20.0, -2.0
    x, y = bx[rows] + a, by[rows] + b
    for v in (x, y):
        v[rng.random((T, C)) < 0.03] = np.nan
    if C > 3:
        y[:, 2], x[:, 3] = np.nan, np.nan
    if C > 5 and T > 90 + LONG_RUN:
        y[20:20 + LONG_RUN, 4], x[90:90 + LONG_RUN, 5] = np.nan, np.nan
    if C > 7 and T > 60:
        x[[7, 33], 6], y[[8, 50], 6] = (900.0, -np.inf), (np.inf, -700.0)
        x[11, 7], x[41, 7] = 148.0, -108.0                              # exactly +-2**7 from the base: out of range
        y[12, 7], y[40, 7] = -2.0 + 128.0 - 2.0 ** -16, -2.0 - 128.0 + 2.0 ** -16      # inside by one unit
    return {"x": x.astype(dtype), "y": y.astype(dtype), "base_x": bx, "base_y": by, "rows": rows, "doy": doys[rows],
            "doys": doys}


def one_class(T):
    return np.zeros(T, dtype=np.int32), 1


def every_step(T):
    """a label that changes every step, K = 3"""
    return (np.arange(T) % 3).astype(np.int32), 3


def long_runs_of_minus_one(T):
    """two classes with runs of -1 of LONG_RUN steps: longer than any lag, so whole histories come from unlabelled steps;
    steps 0 and T - 1 are unlabelled as well"""
    t = np.arange(T)
    k = ((t // 13) % 2).astype(np.int32)
    k[(t // LONG_RUN) % 2 == 1] = -1
    k[[0, T - 1]] = -1
    if T > 3:
        k[1] = 1
    return k, 2


def seasons(T):
    """four classes in runs of 23 steps"""
    return ((np.arange(T) // 23) % 4).astype(np.int32), 4


PATTERNS = (one_class, every_step, long_runs_of_minus_one, seasons)
