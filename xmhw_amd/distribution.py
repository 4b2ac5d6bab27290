"""anomaly_distribution(): per-cell histograms, quantiles and moments of the anomaly -- what the distribution of the anomaly
of a cell looks like, per class of time steps: skewness and kurtosis (why heatwaves and cold spells of one cell are not
mirror images: Sura & Sardeshmukh 2008; and the check on every Gaussian p-value that index_regression(), mhw_composite() and
lag_correlation() print), quantile maps that are not the day-of-year threshold, exceedance probabilities at levels of the
user's choosing.  One pass over the resident series (csrc/kernels_distribution.hip).

The definition (include/xmhw_amd.h, "anomaly_distribution()", states it for the C entries).  Inputs: a series x[T][C], a
base[Dr][C] with row_of_t[T] (one row: a constant per cell), a shift in [0, 24], labels class_of_t[T] in [-1, K), K <= 64,
T < 2**17, bins (lo_q, width_q, B) with |lo_q| <= 2**23, width_q >= 1, 1 <= B <= 256.
    d(t) = (float64(x[t, c]) - base[row_of_t[t], c]) * 2**-shift                            (the scaling is exact)
    NaN is no sample; |d| >= 2**7 (infinities included) is left out and counted in n_range; otherwise the step is VALID
    and q = rint(d * 2**16).  The bin of q is b = floor((q - lo_q) / width_q): b < 0 counts in the UNDER row (row 0),
    b >= B in the OVER row (row B + 1), anything else in row 1 + b.
For every class k and cell c, over the valid steps of class k, exact integers: hist[k, 0 .. B + 1, c] (int32), n (int32),
s1 and s2 (int64: the sums of q and q**2), s3 and s4 (the sums of q**3 and q**4 as 128-bit two's-complement integers: a low
word and a high word), and the smallest and the largest d.  A finish pass on the device walks the histogram of every cell
once: for a probability p_q = rint(p * 2**32) the rank is r = max(1, ceil(p_q * n / 2**32)), and it gives the bin that
holds the r-th smallest valid sample (-1: UNDER, B: OVER, INT32_MIN: no sample), the samples in rows below it and in it;
for a level on the edge e of the bins it gives the samples with b >= e.  The histogram itself stays on the device unless
it is asked for.  Everything is an integer sum, an integer maximum or a function of those: the result does not depend on
the time blocks, the slabs, the launch geometry or the schedule.

Host side here (validation, bins, class labels, slabs, land, derived fields); device side behind distribution_cells()
(compact host series) and distribution_grid() (stacked grids, masked and compacted on the device).
"""
import numpy as np

from ._lib import hip_distribution
from .device import as_xmhw_errors
from .exception import XmhwException
from .lag_correlation import _base_on_ocean
from .series_stage import (Accumulators, cell_stage, check_class_ids, check_steps, class_labels, class_result_labels,
                           dense_ids, grid_layout, ocean_mask, run_cells, run_grid, stage_attrs)

MAX_BINS = 256                  # XMHW_DISTRIBUTION_MAX_BINS (include/xmhw_amd.h)
MAX_CLASSES = 64                # XMHW_DISTRIBUTION_MAX_CLASSES
MAX_QUANTILES = 16              # XMHW_DISTRIBUTION_MAX_QUANTILES
MAX_LEVELS = 8                  # XMHW_DISTRIBUTION_MAX_LEVELS
MAX_STEPS = 1 << 17             # XMHW_DISTRIBUTION_MAX_STEPS: T below it
BITS = 16                       # XMHW_DISTRIBUTION_BITS
RANGE_BITS = 7                  # |d| < 2**7
MAX_SHIFT = 24                  # XMHW_DISTRIBUTION_MAX_SHIFT
ONE = 1 << BITS
NO_SAMPLE = -(1 << 31)          # qbin of a class without a sample
SUMS = ("n", "s1", "s2", "s3", "s4", "kmin", "kmax")
RANKS = ("qbin", "qbelow", "qcount")
FIELDS = SUMS + RANKS + ("n_at_least",)


def _range_texts(shift):
    return {"n_range": ("samples lie 2**(7 + shift) and more from their base (or are infinite) with "
                        f"shift = {shift}: pass a larger shift")}


# ---- validation (mirrors the refusals of the C entries) ----------------------------------------------

def check_shift(shift):
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)):
        raise XmhwException(f"shift should be a whole number, got {shift!r}")
    if not 0 <= int(shift) <= MAX_SHIFT:
        raise XmhwException(f"shift should be in [0, {MAX_SHIFT}], got {int(shift)}")
    return int(shift)


def check_bins(bins):
    """``bins`` = (lo, hi, n) in the units of the shifted anomaly as (lo_q, width_q, B): the edges are rounded to the fixed
    point, and the n bins between them have to be of one whole width"""
    try:
        lo, hi, n = bins
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise XmhwException(f"bins should be (lo, hi, n): two edges and a number of bins, got {bins!r}") from None
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
        raise XmhwException(f"bins should be (lo, hi, n) with n a whole number of bins >= 1, got n = {n!r}")
    n = int(n)
    if n > MAX_BINS:
        raise XmhwException(f"anomaly_distribution handles at most {MAX_BINS} bins, got {n}")
    limit = float(1 << RANGE_BITS)
    if not (-limit <= lo < hi <= limit):
        raise XmhwException(f"bins should be (lo, hi, n) with -{limit:g} <= lo < hi <= {limit:g}, got ({lo!r}, {hi!r})")
    lo_q, hi_q = int(np.rint(lo * ONE)), int(np.rint(hi * ONE))
    span = hi_q - lo_q
    if span % n or span < n:
        width = max(1, (2 * span + n) // (2 * n))
        near = (lo_q + n * width) / ONE
        raise XmhwException(f"the {n} bins between {lo!r} and {hi!r} are not a whole number of units of 2**-{BITS} wide "
                            f"({span} units over {n} bins): the nearest admissible hi is {near!r}")
    return lo_q, span // n, n


def check_levels(levels, lo_q, width_q, B):
    """the levels (units of the shifted anomaly) as edge indices in [0, B]"""
    levels = [float(v) for v in np.atleast_1d(np.asarray(levels, dtype=np.float64))] if np.size(levels) else []
    if len(levels) > MAX_LEVELS:
        raise XmhwException(f"anomaly_distribution handles at most {MAX_LEVELS} levels, got {len(levels)}")
    edges = []
    for v in levels:
        if not np.isfinite(v):
            raise XmhwException(f"levels should be finite, got {v!r}")
        u = int(np.rint(v * ONE)) - lo_q
        e = u // width_q
        if u % width_q or not 0 <= e <= B:
            below = min(max(e, 0), B - 1)
            raise XmhwException(f"level {v!r} is not on a bin edge: the neighbouring edges are "
                                f"{(lo_q + below * width_q) / ONE!r} and {(lo_q + (below + 1) * width_q) / ONE!r}")
        edges.append(e)
    return np.asarray(levels, dtype=np.float64), np.asarray(edges, dtype=np.int32)


def check_quantiles(quantiles):
    """the probabilities as (p float64, p_q uint64 = rint(p * 2**32))"""
    p = np.atleast_1d(np.asarray(quantiles, dtype=np.float64)) if np.size(quantiles) else np.zeros(0)
    if p.ndim != 1:
        raise XmhwException(f"quantiles should be a list of probabilities, got shape {p.shape}")
    if p.shape[0] > MAX_QUANTILES:
        raise XmhwException(f"anomaly_distribution handles at most {MAX_QUANTILES} quantiles, got {p.shape[0]}")
    if p.shape[0] and not (np.all(p >= 0.0) and np.all(p <= 1.0)):
        raise XmhwException(f"quantiles should be probabilities in [0, 1], got {p.tolist()}")
    return p, np.rint(p * 4294967296.0).astype(np.uint64)


def bytes_per_cell_entry(B, P, L):
    """the device accumulators of one class and cell: the histogram above all"""
    return 4 * (B + 2) + 4 + 2 * 8 + 4 * 8 + 2 * 8 + 4 * (3 * P + L)


def check_result_bytes(K, B, P, L, C, max_result_bytes):
    need = bytes_per_cell_entry(B, P, L) * K * C
    if max_result_bytes is not None and need > max_result_bytes:
        raise XmhwException(f"the accumulators of K = {K} classes x C = {C} cells with {B} bins take {need} bytes (the "
                            f"histogram {4 * (B + 2) * K * C}), more than max_result_bytes = {int(max_result_bytes)}: use "
                            "fewer classes, fewer bins or a part of the grid")


def shapes(K, B, P, L, C, histogram=False):
    """the arrays of FIELDS (and ``hist``) for C cells"""
    out = [(K, C)] * 3 + [(K, 2, C)] * 2 + [(K, C)] * 2 + [(K, P, C)] * 3 + [(K, L, C)]
    return out + ([(K, B + 2, C)] if histogram else [])


def ranks(p_q, n):
    """r = max(1, ceil(p_q * n / 2**32)) in 64-bit integers, (K, P, ...) for n (K, ...)"""
    n = np.asarray(n)
    pq = np.asarray(p_q, dtype=np.uint64).reshape((1, -1) + (1,) * (n.ndim - 1))
    r = (pq * n.astype(np.uint64)[:, None] + np.uint64(0xFFFFFFFF)) >> np.uint64(32)
    return np.maximum(r.astype(np.int64), 1)


# ---- the device stage --------------------------------------------------------------------------------

class _Accumulators(Accumulators):
    """One call's arguments and its device accumulators: ``hist`` (K, B + 2, C), which stays on the device unless it is
    asked for, the sums and extremes of SUMS and what the finish pass writes (RANKS, n_at_least)."""

    def __init__(self, classes, K, lo_q, width_q, B, p_q, edges, shift, histogram, max_result_bytes):
        super().__init__()
        self.hd = hip_distribution()
        self.args = (classes, K)
        self.lo_q, self.width_q, self.B = int(lo_q), int(width_q), int(B)
        self.p_q = np.ascontiguousarray(p_q, dtype=np.uint64)
        self.edges = np.ascontiguousarray(edges, dtype=np.int32)
        self.shift = check_shift(shift)
        self.range_texts = _range_texts(self.shift)
        self.histogram, self.max_result_bytes = bool(histogram), max_result_bytes

    def begin(self, T, C):
        """T steps, C ocean cells"""
        check_steps(T, "anomaly_distribution")
        self.classes, self.K = check_class_ids(T, *self.args, MAX_CLASSES, "anomaly_distribution")
        P, L = self.p_q.shape[0], self.edges.shape[0]
        check_result_bytes(self.K, self.B, P, L, C, self.max_result_bytes)
        K, B = self.K, self.B
        table = {"hist": ((K, B + 2, C), np.int32), "n": ((K, C), np.int32), "s1": ((K, C), np.int64),
                 "s2": ((K, C), np.int64), "s3": ((K, 2, C), np.int64), "s4": ((K, 2, C), np.int64),
                 "kmin": ((K, C), np.float64), "kmax": ((K, C), np.float64), "qbin": ((K, P, C), np.int32),
                 "qbelow": ((K, P, C), np.int32), "qcount": ((K, P, C), np.int32), "n_at_least": ((K, L, C), np.int32)}
        self.make(C, table, counters=1)
        with as_xmhw_errors(also="Unsupported"):
            self.hd.distribution_init(K, B, C, *self.ptrs(0, ("hist",) + SUMS), C, self.count.ptr)

    def add_slab(self, slab):
        """One slab (series_stage.Slab), columns k0..k0+n-1 of the accumulators; the base is where the slab carries se."""
        with as_xmhw_errors(also="Unsupported"):
            self.hd.distribution_accumulate(slab.d_ts.ptr, slab.isz, slab.T, slab.n, slab.ld, slab.se_ptr, slab.ldc, slab.D,
                                            slab.rows, self.shift, self.classes, self.K, self.lo_q, self.width_q, self.B,
                                            *self.ptrs(slab.k0, ("hist",) + SUMS), self.C, self.count.ptr)
        self.h.stream_sync(0)                           # the slab's series are freed on the way out

    def finish(self):
        with as_xmhw_errors(also="Unsupported"):
            self.hd.distribution_finish(self.K, self.B, self.C, *self.ptrs(0, ("hist", "n", "kmin", "kmax")), self.p_q,
                                        self.edges, *self.ptrs(0, RANKS + ("n_at_least",)), self.C)

    def result(self):
        """(the arrays of FIELDS and, where asked for, hist; {n_range})"""
        if self.C != 0:
            self.finish()
        self.h.stream_sync(0)
        return self.read(FIELDS + (("hist",) if self.histogram else ())), dict(zip(self.range_texts, self.counts()))


def _bytes_per_cell(T, isz, D):
    return T * isz + 2 * D * 8 + 64


def distribution_cells(ts, base, doy, doys, classes, K, lo_q, width_q, B, p_q, edges, shift=0, return_histogram=False,
                       max_batch_bytes=64 << 30, pad=None, counters=None, max_result_bytes=None):
    """The device stage for a dense (T, C) series: a base (Dr, C) with the labels doy (T,) / doys (Dr,) that pair steps and
    base rows as in detect_front.detect_cells, classes (T,) int labels in [-1, K), bins (lo_q, width_q, B), probabilities
    p_q (P,) uint64 and edge indices edges (L,).  Returns the arrays of FIELDS -- n, s1, s2 (K, C); s3, s4 (K, 2, C): low
    and high words; kmin, kmax (K, C) float64; qbin, qbelow, qcount (K, P, C); n_at_least (K, L, C) -- and, with
    ``return_histogram``, hist (K, B + 2, C).  Cells go through the device in batches below max_batch_bytes; the sums are
    integers, so the batch size does not change a single bit.  Raises if a sample is out of range (module docstring);
    with ``counters`` (a dict) it stores ``n_range`` there instead."""
    from .device import native_float
    acc = _Accumulators(classes, K, lo_q, width_q, B, p_q, edges, shift, return_histogram, max_result_bytes)
    return run_cells(acc, native_float(ts), base, base, doy, doys, _bytes_per_cell, max_batch_bytes, pad, counters)


def distribution_grid(stacked, anynans, base, doy, doys, classes, K, lo_q, width_q, B, p_q, edges, shift=0,
                      return_histogram=False, max_batch_bytes=None, clim_stacked=False, pad=None, counters=None,
                      max_result_bytes=None):
    """distribution_cells() for an UNCOMPACTED stacked host series (T, N): the land mask and the compaction run on the
    device slab by slab (series_stage.walk_grid).  Returns the arrays over the ocean cells and keep[N]."""
    acc = _Accumulators(classes, K, lo_q, width_q, B, p_q, edges, shift, return_histogram, max_result_bytes)
    out, keep = run_grid(acc, stacked, anynans, base, base, doy, doys, lambda T, D: 4 * D * 8 + 64, max_batch_bytes,
                         clim_stacked, pad, counters)
    return out + (keep,)


# ---- the result --------------------------------------------------------------------------------------

def wide(words):
    """(K, 2, ...) int64 low and high words as an object array of Python integers (K, ...)"""
    words = np.asarray(words, dtype=np.int64)
    lo = words[:, 0].view(np.uint64).astype(object)
    return words[:, 1].astype(object) * (1 << 64) + lo


def _as_float(a):
    return np.asarray(a, dtype=object).astype(np.float64)


class DistributionDataset:
    """What anomaly_distribution() returns, as plain arrays over (klass, *spatial dims).

    klass (K,) the class labels (sorted non-negative labels found), shift, bins (lo_q, width_q, B) in units of
    2**-16 of the shifted anomaly, bin_edges (B + 1,), probability (P,), level (L,).
    Raw integers: n int32, s1 and s2 int64, s3 and s4 (klass, 2, ...) int64 low and high words (module docstring).
    Derived float64, in the units of the field (the shifted anomaly times 2**shift), from the exact integers -- the
    central moments are formed from the raw power sums in Python integers, so the cancellation happens in integers, and
    rounded to float64 at the end; with N = n, S_i the power sums, A2 = N S2 - S1**2, A3 = N**2 S3 - 3 N S1 S2 + 2 S1**3,
    A4 = N**3 S4 - 4 N**2 S1 S3 + 6 N S1**2 S2 - 3 S1**4:
        mean       S1 / N                          variance   A2 / N**2 (of the population: no N - 1)
        skewness   A3 / A2**1.5                    kurtosis   A4 / A2**2 - 3 (excess)
        minimum, maximum                           the smallest and the largest valid anomaly itself, not quantised
    mean, variance, minimum and maximum are NaN where n == 0, skewness and kurtosis where n < 2 or the variance is zero.
        quantile   (klass, quantile, ...) lo + (b + (r - below - 0.5) / h_b) * width: the rank r of the probability
                   among the n samples, b the bin that holds it, h_b its count, ``below`` the samples in lower rows -- the
                   samples of a bin taken as evenly spread over it; NaN where the rank falls into UNDER or OVER or n == 0
        quantile_bin    (klass, quantile, ...) int32: b; -1 = UNDER, B = OVER, -2**31 = no sample
        exceedance      (klass, level, ...) int32: the valid samples at or above the level (an edge of the bins)
        exceedance_probability   exceedance / n, NaN where n == 0
        histogram  (klass, B + 2, ...) int32 with return_histogram=True, else None: rows UNDER, the B bins, OVER
    Land: grid lines without an ocean cell are dropped, as in ClassDaysDataset; the float fields are NaN on the remaining
    land cells, integer fields are 0 there (quantile_bin -2**31) and come with the boolean ``keep`` (...) mask."""

    def __init__(self, klass, n, s1, s2, s3, s4, minimum, maximum, qbin, qbelow, qcount, n_at_least, keep, sdims, coords,
                 bins, probability, level, shift=0, histogram=None, tdim="time", attrs=None):
        self.klass = np.asarray(klass)
        self.n, self.s1, self.s2, self.s3, self.s4 = n, s1, s2, s3, s4
        self.keep, self.sdims, self.coords = keep, tuple(sdims), dict(coords)
        self.lo_q, self.width_q, self.B = (int(v) for v in bins)
        self.probability, self.level = np.asarray(probability, dtype=np.float64), np.asarray(level, dtype=np.float64)
        self.shift, self.histogram = int(shift), histogram
        self.tdim, self.attrs = tdim, dict(attrs or {})
        unit = 2.0 ** (self.shift - BITS)
        scale = 2.0 ** self.shift
        self.bin_edges = (self.lo_q + self.width_q * np.arange(self.B + 1)) / ONE * scale
        none = np.asarray(n) == 0
        self.minimum = np.where(none, np.nan, np.asarray(minimum, dtype=np.float64) * scale)
        self.maximum = np.where(none, np.nan, np.asarray(maximum, dtype=np.float64) * scale)
        # the power sums as Python integers
        N = np.asarray(n).astype(object)
        S1, S2, S3, S4 = np.asarray(s1).astype(object), np.asarray(s2).astype(object), wide(s3), wide(s4)
        A2 = N * S2 - S1 * S1
        A3 = N * N * S3 - 3 * N * S1 * S2 + 2 * S1 * S1 * S1
        A4 = N * N * N * S4 - 4 * N * N * S1 * S3 + 6 * N * S1 * S1 * S2 - 3 * S1 * S1 * S1 * S1
        nf = np.asarray(n, dtype=np.float64)
        a2 = _as_float(A2)
        flat = (np.asarray(n) < 2) | (a2 <= 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.mean = np.where(none, np.nan, _as_float(S1) / nf * unit)
            self._m2 = np.where(none, np.nan, a2 / (nf * nf))                  # central moments in units of 2**-16
            self._m3 = np.where(none, np.nan, _as_float(A3) / nf ** 3)
            self._m4 = np.where(none, np.nan, _as_float(A4) / nf ** 4)
            self.variance = self._m2 * unit * unit
            self.skewness = np.where(flat, np.nan, _as_float(A3) / a2 ** 1.5)
            self.kurtosis = np.where(flat, np.nan, _as_float(A4) / _as_float(A2 * A2) - 3.0)
            # quantiles: the rank inside its bin
            self.quantile_bin = qbin
            inside = (np.asarray(qbin) >= 0) & (np.asarray(qbin) < self.B)
            r = ranks(np.rint(self.probability * 4294967296.0).astype(np.uint64), np.asarray(n))
            frac = (r - qbelow - 0.5) / np.where(inside, qcount, 1)
            q = (self.lo_q + (qbin + frac) * self.width_q) / ONE * scale
            self.quantile = np.where(inside, q, np.nan)
            self.exceedance = n_at_least
            self.exceedance_probability = np.where(none[:, None], np.nan, n_at_least / np.where(none, 1.0, nf)[:, None])

    def quantisation_bound(self):
        """What the fixed point costs each derived field, as a dict of bounds on |field - the same statistic of the
        unquantised anomalies|, in the units of the field.  A sample enters as q = rint(d * 2**16): it is off by at most
        the half unit h = 2**(shift - 17).  With s, m2, m3, m4 the standard deviation and central moments of the
        quantised samples (arrays like ``mean``):
            unit        h itself                       minimum, maximum   0: they are the samples themselves
            mean        h                              quantile           width + h: the bin holds the order statistic
            variance    D2 = 2 h s + h**2
            skewness    D3 / L2**1.5 + |m3| (L2**-1.5 - m2**-1.5) with D3 = 6 h m2 + 12 h**2 s + 8 h**3, L2 = m2 - D2
            kurtosis    D4 / L2**2 + m4 (L2**-2 - m2**-2) with D4 = 8 h m4**0.75 + 24 h**2 m2 + 32 h**3 s + 16 h**4
        (expand the central moment of q - e around q with |e - mean(e)| <= 2 h, and mean|w|**3 <= m4**0.75); infinite
        where L2 <= 0: the spread of the cell is not above the resolution."""
        h = 2.0 ** (self.shift - BITS - 1)
        u = 2.0 ** (self.shift - BITS)
        with np.errstate(divide="ignore", invalid="ignore"):
            m2, m3, m4 = self._m2 * u ** 2, self._m3 * u ** 3, self._m4 * u ** 4
            s = np.sqrt(m2)
            d2 = 2 * h * s + h * h
            d3 = 6 * h * m2 + 12 * h * h * s + 8 * h ** 3
            d4 = 8 * h * m4 ** 0.75 + 24 * h * h * m2 + 32 * h ** 3 * s + 16 * h ** 4
            l2 = m2 - d2
            ok = l2 > 0.0
            l2 = np.where(ok, l2, np.nan)
            skew = np.where(ok, d3 / l2 ** 1.5 + np.abs(m3) * (l2 ** -1.5 - m2 ** -1.5), np.inf)
            kurt = np.where(ok, d4 / l2 ** 2 + m4 * (l2 ** -2 - m2 ** -2), np.inf)
        nan = np.isnan(m2)
        return {"unit": h, "mean": h, "minimum": 0.0, "maximum": 0.0, "quantile": self.width_q / ONE * 2.0 ** self.shift + h,
                "variance": d2, "skewness": np.where(nan, np.nan, skew), "kurtosis": np.where(nan, np.nan, kurt)}

    def to_xarray(self):
        import xarray as xr
        cell = ("klass",) + self.sdims
        data = {k: (cell, getattr(self, k)) for k in ("n", "s1", "s2", "mean", "variance", "skewness", "kurtosis", "minimum",
                                                      "maximum")}
        data.update({k: (("klass", "word") + self.sdims, getattr(self, k)) for k in ("s3", "s4")})
        data.update({k: (("klass", "quantile") + self.sdims, getattr(self, k)) for k in ("quantile", "quantile_bin")})
        data.update({k: (("klass", "level") + self.sdims, getattr(self, k)) for k in ("exceedance", "exceedance_probability")})
        if self.histogram is not None:
            data["histogram"] = (("klass", "row") + self.sdims, self.histogram)
        data.update(keep=(self.sdims, self.keep), bin_edges=(("edge",), self.bin_edges))
        coords = dict({"klass": self.klass, "quantile": self.probability, "level": self.level},
                      **{d: self.coords[d] for d in self.sdims if d in self.coords})
        return xr.Dataset(data, coords=coords, attrs=dict(self.attrs, shift=self.shift, lo_q=self.lo_q, width_q=self.width_q,
                                                          bins=self.B))


# ---- the public function -----------------------------------------------------------------------------

def anomaly_distribution(temp, base=None, bins=(-8.0, 8.0, 128), quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), levels=(),
                         classes="all", shift=0, tdim="time", maxPadLength=None, anynans=False, return_histogram=False,
                         max_batch_bytes=None, max_result_bytes=8 << 30, _compute=None):
    """The distribution of ``temp - base`` per cell and class of time steps: histogram, moments, quantiles and
    exceedance counts, from exact integer sums.

    ``temp``, ``base``, ``classes`` and ``shift`` are taken as lag_correlation() takes ``x``, ``base_x``, ``classes`` and
    ``shift_x``: land masking, padding, a constant base per cell or a ('doy', ...) climatology on the grid of ``temp``, a
    base of None is zero; at most 64 classes, a label of -1 counts nowhere; samples enter as d = (temp - base) *
    2**-shift and must then lie inside (-2**7, 2**7), float32 or float64.
    ``bins`` = (lo, hi, n): n <= 256 bins of one width between lo and hi, in the units of the shifted anomaly d; the
    edges are rounded to multiples of 2**-16 and the width has to be a whole number of those: the call raises and names
    the nearest admissible ``hi`` otherwise.  Samples below lo and at or above hi are counted in rows of their own.
    ``quantiles``: at most 16 probabilities in [0, 1].  ``levels``: at most 8 levels in the units of d, each on an edge
    of the bins.  ``return_histogram``: read the histogram rows back as well.  The device accumulators -- the histogram
    above all, K (n + 2) C int32 -- are checked against ``max_result_bytes`` before anything is allocated.

    Returns a DistributionDataset.  Raises if a sample is out of range.  ``_compute``: a stand-in for
    distribution_cells() (host tests)."""
    shift = check_shift(shift)
    lo_q, width_q, B = check_bins(bins)
    level, edges = check_levels(levels, lo_q, width_q, B)
    prob, p_q = check_quantiles(quantiles)
    P, L = prob.shape[0], level.shape[0]
    layout = grid_layout(temp, tdim)
    coords, _, dims, point, sdims, sshape, N = layout
    time = np.asarray(coords[tdim])
    check_steps(time.shape[0], "anomaly_distribution")
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "anomaly_distribution", "classes")
    b = _base_on_ocean(base, ocean_mask(temp, dims, tdim, point, anynans), point, sdims, sshape, coords, "base")
    more = (kid, K, lo_q, width_q, B, p_q, edges)
    options = dict(shift=shift, return_histogram=return_histogram, max_result_bytes=max_result_bytes)

    def on_cells(host_keep, ts, sec, thc, doy, doys, _options, **extra):
        check_result_bytes(K, B, P, L, ts.shape[1], max_result_bytes)
        return (_compute or distribution_cells)(ts, sec, doy, doys, *more, **options, **extra)

    f, arrays, mhw = cell_stage(
        "anomaly distribution", temp, b, b, layout, tdim, on_cells,
        lambda stacked, anynans_, sec, thc, doy, doys, _options, **extra:
            distribution_grid(stacked, anynans_, sec, doy, doys, *more, **options, **extra),
        lambda C: shapes(K, B, P, L, C, return_histogram), _range_texts(shift), maxPadLength=maxPadLength, anynans=anynans,
        _compute=_compute, max_batch_bytes=max_batch_bytes)
    got = dict(zip(FIELDS + ("hist",), arrays))
    raw = {k: f.place(got[k], 0, np.int32 if k == "n" else np.int64) for k in ("n", "s1", "s2", "s3", "s4")}
    ext = {k: f.place(got[k], np.nan, np.float64) for k in ("kmin", "kmax")}
    rk = {k: f.place(got[k], NO_SAMPLE if k == "qbin" else 0, np.int32) for k in RANKS + ("n_at_least",)}
    hist = f.place(got["hist"], 0, np.int32) if return_histogram else None
    return DistributionDataset(class_result_labels(found), raw["n"], raw["s1"], raw["s2"], raw["s3"], raw["s4"], ext["kmin"],
                               ext["kmax"], rk["qbin"], rk["qbelow"], rk["qcount"], rk["n_at_least"], f.keep, f.sdims,
                               f.coords, (lo_q, width_q, B), prob, level, shift, hist, tdim, stage_attrs(classes, mhw))
