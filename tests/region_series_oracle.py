"""region_series() in plain numpy int64: rint, a mask and np.add.at.  TEST INFRASTRUCTURE ONLY.

For every step t and region r, over the cells c with region[c] == r whose sample is not NaN and lies within 2**7 of
x0: acc[t, r] += (1, wi[c], wi[c] * rint((float64(ts[t, c]) - x0) * 2**16)).  A non-NaN sample of such a cell at 2**7
and more from x0, or infinite, is left out and counted in n_range."""
import numpy as np

SERIES_BITS = 16
RANGE = 128.0


def quantised(ts, x0=0.0):
    """(xq int64 (T, C) with 0 where the sample does not count, ok mask, out-of-range mask)"""
    d = np.asarray(ts).astype(np.float64) - float(x0)
    valid = ~np.isnan(d)
    with np.errstate(invalid="ignore"):
        inside = np.abs(d) < RANGE                      # False for +-inf
    ok = valid & inside
    xq = np.rint(np.where(ok, d, 0.0) * 65536.0).astype(np.int64)
    return xq, ok, valid & ~inside


def region_cells(ts, wi, region, R, x0=0.0):
    """(acc int64 (T, R, 3), n_range)"""
    ts = np.asarray(ts)
    T, C = ts.shape
    wi = np.asarray(wi, dtype=np.int64)
    region = np.asarray(region, dtype=np.int64)
    assert wi.shape == (C,) and region.shape == (C,) and (C == 0 or (region.min() >= -1 and region.max() < R))
    xq, ok, out = quantised(ts, x0)
    live = region >= 0
    ok = ok & live[None, :]
    n_range = int((out & live[None, :]).sum())
    acc = np.zeros((T, R, 3), dtype=np.int64)
    where = (np.arange(T)[:, None], np.where(live, region, 0)[None, :])
    one = ok.astype(np.int64)
    np.add.at(acc[:, :, 0], where, one)
    np.add.at(acc[:, :, 1], where, one * wi[None, :])
    np.add.at(acc[:, :, 2], where, one * wi[None, :] * xq)
    return acc, n_range


def mean_of(acc, x0=0.0):
    """offset + xsum_q / (wsum_i * 2**16), NaN where wsum_i == 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        m = float(x0) + acc[..., 2].astype(np.float64) / (acc[..., 1].astype(np.float64) * 2.0 ** SERIES_BITS)
    return np.where(acc[..., 1] > 0, m, np.nan)
