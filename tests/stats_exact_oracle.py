"""Exact reference of block_average()'s device stage (csrc/kernels_stats.hip), one cell and one bin at a
time.  TEST INFRASTRUCTURE ONLY: plain Python / numpy, no device code.

Semantics (header of kernels_stats.hip, oracle/stats_oracle.py): ``count`` = number of non-NaN values;
``sum`` / ``mean`` / ``max`` / ``min`` skip NaN; an empty or all-NaN group gives NaN for mean / max / min and
0.0 for sum and count.  Unlike stats_oracle (np.mean: a pairwise sum) the sums here are ``math.fsum``, exactly
rounded, and every mean / sum entry comes with its ``n`` and ``S = fsum(|x_i|)``, from which the bound of a
sequential float64 sum in ANY order follows -- a column that changes sign has no meaningful relative tolerance:

    count, max, min, day counts, total_days    bit-equal (NaN positions equal)
    sum                                        |got - ref| <= n * 2**-52 * S
    mean                                       |got - ref| <= 2**-52 * S

(first order a sequential sum of n terms is off by at most (n - 1) * 2**-53 * S; the factor 2 covers the final
division and the second-order term.)  An entry with n <= 1 has S-bound 0 by definition here: bit-equal.

Event binning: ``pos = table[e, mtime column]``; an event is in no group when pos is NaN, < 0, >= T or when
``bin_of_t[int(pos)]`` lies outside [0, nbins).  Time statistics take the steps with bin_of_t[t] in range;
float32 series are widened to float64 first (exact); day counts are ``cats == k`` for k = 1..4 (NaN nowhere).
"""
import math

import numpy as np
import numpy.testing as npt

import stats_oracle as so
from xmhw_amd.detect_front import EVENT_COLUMNS

EPS = 2.0 ** -52
# (source column in the event table, aggregation) of the 15 statistics, from the aggregation dictionary
EVENT_AGG = [(EVENT_COLUMNS.index(src), how) for _, src, how in so.MHW_AGG]
EVENT_SOURCE_COLUMNS = sorted({c for c, _ in EVENT_AGG})


def agg(values, how):
    """One group: (value, n, S) with n = number of non-NaN values, S = fsum(|x|) over them."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)].tolist()
    n = len(v)
    if how == "count":
        return float(n), n, 0.0
    S = math.fsum(abs(x) for x in v)
    if how == "sum":
        return (math.fsum(v) if n else 0.0), n, S
    if n == 0:
        return math.nan, 0, 0.0
    if how == "mean":
        return math.fsum(v) / n, n, S
    return (max(v) if how == "max" else min(v)), n, S


def event_bins(table, bin_of_t, nbins, mtime_col):
    """bin of every event, -1 where it is in no group"""
    pos = np.asarray(table, dtype=np.float64)[:, mtime_col]
    b = np.full(pos.shape[0], -1, dtype=np.int64)
    ok = (pos >= 0) & (pos < len(bin_of_t))              # (a NaN position compares False)
    b[ok] = np.asarray(bin_of_t)[pos[ok].astype(np.int64)]
    b[(b < 0) | (b >= nbins)] = -1
    return b


def event_stats(table, offsets, bin_of_t, nbins, mtime_col):
    """The 15 event statistics of every (bin, cell): dict(val, n, S), each (15, nbins, C)."""
    C = len(offsets) - 1
    ns = len(EVENT_AGG)
    val = np.empty((ns, nbins, C))
    for j, (_, how) in enumerate(EVENT_AGG):
        val[j] = 0.0 if how in ("count", "sum") else np.nan
    n = np.zeros((ns, nbins, C), dtype=np.int64)
    S = np.zeros((ns, nbins, C))
    b = event_bins(table, bin_of_t, nbins, mtime_col)
    for c in range(C):
        lo, hi = int(offsets[c]), int(offsets[c + 1])
        bc = b[lo:hi]
        for k in np.unique(bc[bc >= 0]):
            rows = table[lo:hi][bc == k]
            for j, (src, how) in enumerate(EVENT_AGG):
                val[j, k, c], n[j, k, c], S[j, k, c] = agg(rows[:, src], how)
    return dict(val=val, n=n, S=S)


def time_stats(ts, cats, bin_of_t, nbins):
    """ts_mean, ts_max, ts_min (+ the four day counts with cats) of every (bin, cell): dict(val (3 or 7, nbins, C),
    n, S (nbins, C): those of ts_mean)."""
    x = np.asarray(ts).astype(np.float64)
    T, C = x.shape
    bin_of_t = np.asarray(bin_of_t)
    val = np.full((3 if cats is None else 7, nbins, C), np.nan)
    n = np.zeros((nbins, C), dtype=np.int64)
    S = np.zeros((nbins, C))
    for k in range(nbins):
        sel = bin_of_t == k
        xs = x[sel]
        for c in range(C):
            val[0, k, c], n[k, c], S[k, c] = agg(xs[:, c], "mean")
            val[1, k, c] = agg(xs[:, c], "max")[0]
            val[2, k, c] = agg(xs[:, c], "min")[0]
        if cats is not None:
            ks = np.asarray(cats, dtype=np.float64)[sel]
            for d in (1, 2, 3, 4):
                val[2 + d, k] = (ks == d).sum(axis=0)
    return dict(val=val, n=n, S=S)


def _assert_bounded(got, ref, bound, n, what):
    """NaN positions equal, |got - ref| <= bound, bit-equal where n <= 1"""
    npt.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what}: NaN positions")
    fin = ~np.isnan(ref)
    err = np.abs(got[fin] - ref[fin])
    bad = err > bound[fin]
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {int(fin.sum())} entries beyond the bound; worst error "
                           f"{err[bad].max():.3e} against a bound of {bound[fin][bad].min():.3e}")
    one = n <= 1
    npt.assert_array_equal(got[one], ref[one], err_msg=f"{what}: entries of at most one value")


def assert_event_stats(got, ref, what=""):
    """got (15, nbins, C) against event_stats()'s result under the bounds of the module docstring"""
    assert got.shape == ref["val"].shape, (got.shape, ref["val"].shape)
    for j, (name, _, how) in enumerate(so.MHW_AGG):
        label = f"{what} {name}"
        if how == "sum":
            _assert_bounded(got[j], ref["val"][j], ref["n"][j] * EPS * ref["S"][j], ref["n"][j], label)
        elif how == "mean":
            _assert_bounded(got[j], ref["val"][j], EPS * ref["S"][j], ref["n"][j], label)
        else:
            npt.assert_array_equal(got[j], ref["val"][j], err_msg=label)


def assert_time_stats(got, ref, what=""):
    """got (3 or 7, nbins, C) against time_stats()'s result"""
    assert got.shape == ref["val"].shape, (got.shape, ref["val"].shape)
    _assert_bounded(got[0], ref["val"][0], EPS * ref["S"], ref["n"], f"{what} ts_mean")
    for j in range(1, got.shape[0]):
        npt.assert_array_equal(got[j], ref["val"][j], err_msg=f"{what} {so.TIME_STATS[j]}")
