"""The case generators and class patterns shared by the host and the GPU tests of heat_stress().  TEST INFRASTRUCTURE
ONLY."""
import numpy as np

ONE = 65536


def synthetic(T, C, dtype, seed, W, D=1, nan_frac=0.02, cold=False, marks=(64,)):
    """A (T, C) series around a (D, C) baseline with what the window has to get right: hot runs longer than W (and than
    the blocks of ``marks`` steps), single hot steps, samples exactly on the floor of 1.0 and one float below it, NaN
    runs that straddle the multiples of every mark, NaN base cells.  Returns ts, base, rows (T,), doy, doys."""
    rng = np.random.default_rng(seed)
    base = np.round(18.0 + 6.0 * rng.random((D, C)), 2)
    doys = np.arange(1, D + 1) if D > 1 else np.zeros(1, dtype=np.int64)
    rows = ((np.arange(T) + 37) % D).astype(np.int32)
    doy = doys[rows]
    h = rng.normal(-0.4, 0.9, (T, C))
    for c in range(C):                                      # hot runs, some longer than the window and a block
        for _ in range(1 + T // 150):
            s, n = int(rng.integers(0, T)), int(rng.integers(1, 2 * W + 70))
            h[s:s + n, c] = 1.0 + 3.0 * rng.random()
    sign = -1.0 if cold else 1.0
    ts = (base[rows] + sign * h).astype(dtype)
    on = rng.random((T, C)) < 0.01                           # exactly on the floor, and the next float below it
    below = rng.random((T, C)) < 0.01
    ts = np.where(on, (base[rows] + sign * 1.0).astype(dtype), ts)
    edge = np.nextafter((base[rows] + sign * 1.0).astype(dtype), np.asarray(-sign * np.inf, dtype=dtype))
    ts = np.where(below & ~on, edge, ts).astype(dtype)
    for m in marks:                                          # NaN runs across the block starts
        for s in range(m, T, max(m, 1)):
            cols = rng.random(C) < 0.3
            ts[max(0, s - 3):s + 4, cols] = np.nan
    ts[rng.random((T, C)) < nan_frac] = np.nan
    if C > 3:
        base[:, 3] = np.nan                                  # a cell without a baseline: never valid
    return {"ts": ts, "base": base, "rows": rows, "doy": doy, "doys": doys}


def one_class(T):
    return np.zeros(T, dtype=np.int32), 1


def per_year(T):
    """classes in runs of 100 steps"""
    return (np.arange(T) // 100).astype(np.int32), max((T - 1) // 100 + 1, 1)


def every_step(T):
    """Labels that change every step, some -1: the flush-per-step worst case."""
    return np.random.default_rng(11).integers(-1, 7, T).astype(np.int32), 7


def runs_of_minus_one(T):
    k = ((np.arange(T) // 13) % 3).astype(np.int32)
    k[(np.arange(T) // 29) % 2 == 1] = -1
    return k, 3


PATTERNS = (one_class, per_year, every_step, runs_of_minus_one)


def levels(L, unit=7.0):
    """L ascending levels that a window of hot steps of 1..4 degrees reaches for small L and does not for the last"""
    return np.rint(np.array([0.5, 1.0, 2.0, 4.0, 8.0, 400.0][:L]) * unit * ONE).astype(np.int64)


def check_case(want):
    """On the oracle's side: a case without hot steps, without valid steps that are not hot, or whose first level is
    never reached proves nothing."""
    n_valid, n_hot = want["counts"][:, 0].sum(), want["counts"][:, 1].sum()
    assert 0 < n_hot < n_valid, "hot steps and other valid steps are both needed"
    assert want["peak_q"].max() > 0 and (want["peak_q"] > 0).any()
