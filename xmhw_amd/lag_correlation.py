"""lag_correlation(): per-cell lagged auto- and cross-correlation -- the memory of the anomaly of a cell (its
autocorrelation function, e-folding time, integral time scale and the effective sample size behind every significance
test of a map: Holbrook et al. 2019; Jacox et al. 2022) and the lagged correlation of two fields in the same cell (net
heat flux, wind stress or mixed-layer depth against the SST anomaly, the forcing leading by 0 .. 60 days).
index_regression() relates a cell to an index shared by all cells and carries one lag-1 pair; mhw_composite() sees a
second field only near events; this is the reduction over the pairs (x(t), y(t - l)) of a cell, per class of time steps
and lag.  One pass over two resident series (csrc/kernels_lagcorr.hip).

The definition (include/xmhw_amd.h, "lag_correlation()", states it for the C entries).  Inputs: series x[T][C] and y[T][C]
(y may be x), bases base_x[Dr][C] and base_y[Dr][C] with one row_of_t[T] (one row: a constant per cell), shifts in
[0, 24], labels class_of_t[T] in [-1, K), K <= 64, a largest lag L in [0, 63], T < 2**17.
    ax(t) = (float64(x[t, c]) - base_x[row_of_t[t], c]) * 2**-shift_x, likewise ay        (the scaling is exact)
    a value is VALID iff it is not NaN and |a| < 2**7; q = rint(a * 2**16).
For every cell c, every step t with k = class_of_t[t] >= 0, every lag l in [0, L] with t - l >= 0 and ax(t), ay(t - l)
both valid:
    n[k, l, c] += 1 (int32);  sx += qx(t), sy += qy(t - l), sxx += qx(t)**2, syy += qy(t - l)**2, sxy += qx(t) qy(t - l)
    (int64).
The class of a pair is that of its LATER step; the earlier step may be of any class, -1 included.  All six sums run over
the valid pairs alone (pairwise deletion), so Pearson's r of every lag is a true correlation.  n_range counts, per field,
the steps whose anomaly is not NaN and out of range (x: on the steps of class >= 0; y: on every step).  Everything is an
integer sum: the result does not depend on the time blocks, the slabs, the launch geometry or the schedule.

Host side here (validation, the second field, class labels, slabs, land, derived fields); device side behind
lag_corr_cells() (compact host series) and lag_corr_grid() (stacked grids, x masked and compacted on the device and y
gathered there by the same mask).
"""
import math

import numpy as np

from ._lib import hip_lagcorr
from .api import GridSeries, _from_xarray, _is_xarray
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .series_stage import (Accumulators, base_series, cell_stage, check_class_ids, check_same_frame, check_steps, class_labels,
                           class_result_labels, dense_ids, grid_layout, ocean_mask, run_cells, run_grid, stage_attrs,
                           zero_base)
from .trend import _t_two_sided, p_two_sided                 # noqa: F401  (_t_two_sided: the host tests reach it here)

MAX_LAG = 63                    # XMHW_LAG_CORR_MAX_LAG (include/xmhw_amd.h)
MAX_CLASSES = 64                # XMHW_LAG_CORR_MAX_CLASSES
MAX_STEPS = 1 << 17             # XMHW_LAG_CORR_MAX_STEPS: T below it
BITS = 16                       # XMHW_LAG_CORR_BITS
RANGE_BITS = 7                  # |a| < 2**7
MAX_SHIFT = 24                  # XMHW_LAG_CORR_MAX_SHIFT
FIELDS = ("n", "sx", "sy", "sxx", "syy", "sxy")
_SWAPPED = ("n", "sy", "sx", "syy", "sxx", "sxy")       # the same sums with the roles of the two fields exchanged
BYTES_PER_ENTRY = 44            # int32 n and five int64 sums


def _range_texts(shift_x, shift_y):
    """the refusal of out-of-range samples of each field, by the key of its counter"""
    return {f"n_range_{name}": (f"samples of {name} lie 2**(7 + shift_{name}) and more from their base (or are infinite) with "
                                f"shift_{name} = {shift}: pass a larger shift_{name} (heat flux in W m-2 needs a shift of 4 or so)")
            for name, shift in (("x", shift_x), ("y", shift_y))}


# ---- validation (mirrors the refusals of the C entries) ----------------------------------------------

def check_lags(lags):
    """(lo, hi) as Python ints with lo <= 0 <= hi"""
    try:
        lo, hi = lags
    except (TypeError, ValueError):
        raise XmhwException(f"lags should be a pair (lo, hi) of whole numbers of steps, got {lags!r}") from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise XmhwException(f"lags should be a pair (lo, hi) of whole numbers of steps, got {lags!r}")
    lo, hi = int(lo), int(hi)
    if lo > 0 or hi < 0:
        raise XmhwException(f"lags should be (lo, hi) with lo <= 0 <= hi, got ({lo}, {hi})")
    if hi > MAX_LAG or -lo > MAX_LAG:
        raise XmhwException(f"lag_correlation handles lags of at most {MAX_LAG} steps either way, got ({lo}, {hi}): a "
                            "coarser series reaches further")
    return lo, hi


def check_shifts(shift_x, shift_y):
    for name, v in (("shift_x", shift_x), ("shift_y", shift_y)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise XmhwException(f"{name} should be a whole number, got {v!r}")
        if not 0 <= int(v) <= MAX_SHIFT:
            raise XmhwException(f"{name} should be in [0, {MAX_SHIFT}], got {int(v)}")
    return int(shift_x), int(shift_y)


def check_result_bytes(K, lo, hi, C, max_result_bytes):
    """the (K, lags, C) accumulators, 44 bytes an entry, live on the device across the slabs and come back whole"""
    need = BYTES_PER_ENTRY * K * (hi - lo + 1) * C
    if max_result_bytes is not None and need > max_result_bytes:
        raise XmhwException(f"the sums of K = {K} classes x {hi - lo + 1} lags ({lo} .. {hi}) x C = {C} cells take {need} "
                            f"bytes, more than max_result_bytes = {int(max_result_bytes)}: use fewer classes, fewer lags "
                            "or a part of the grid")


def assemble(first, second, lo, hi, auto):
    """The six arrays over the lags lo .. hi from the device passes: ``first`` over the lags 0 .. hi of (x, y);
    ``second`` over the lags 0 .. -lo of (y, x), or None.  A negative lag -l pairs x(t) with y(t + l): the pass with the
    roles exchanged, its sums renamed.  For an autocorrelation (``auto``) that pass is the first one itself."""
    first = dict(zip(FIELDS, first))
    if lo == 0:
        return tuple(first[k] for k in FIELDS)
    other = first if auto else dict(zip(FIELDS, second))
    return tuple(np.concatenate([other[s][:, -lo:0:-1], first[k][:, :hi + 1]], axis=1) for k, s in zip(FIELDS, _SWAPPED))


# ---- the device stage --------------------------------------------------------------------------------

class _Accumulators(Accumulators):
    """One call's arguments and its device accumulators (FIELDS, (K, L + 1, C)) with the two range counters of the pass
    over (x, y); for negative lags of two fields ``back`` is a second set of the same table, in the same scope, for the
    pass over (y, x).  ``second(slab)`` gives the slab's columns of y on the device, or None for an autocorrelation."""

    def __init__(self, second, classes, K, lo, hi, shift_x, shift_y, max_result_bytes):
        super().__init__()
        self.hl = hip_lagcorr()
        self.second, self.args = second, (classes, K)
        self.lo, self.hi = check_lags((lo, hi))
        self.shift_x, self.shift_y = check_shifts(shift_x, shift_y)
        self.range_texts = _range_texts(self.shift_x, self.shift_y)
        self.max_result_bytes = max_result_bytes

    def begin(self, T, C):
        """T steps, C ocean cells"""
        check_steps(T, "lag_correlation")
        self.classes, self.K = check_class_ids(T, *self.args, MAX_CLASSES, "lag_correlation")
        check_result_bytes(self.K, self.lo, self.hi, C, self.max_result_bytes)
        # the largest lag of each pass: (x, y), and (y, x) where two fields have negative lags; the one pass of an
        # autocorrelation serves both signs
        two = self.second is not None and self.lo < 0
        self.L = self.hi if self.second is not None else max(self.hi, -self.lo)
        self.passes = [self]
        if two:
            self.back = Accumulators(self._scope)
            self.back.L = -self.lo
            self.passes.append(self.back)
        for p in self.passes:
            p.make(C, {k: ((self.K, p.L + 1, C), np.int32 if k == "n" else np.int64) for k in FIELDS}, counters=2)
            with as_xmhw_errors(also="Unsupported"):
                self.hl.lag_corr_init(self.K, p.L, C, *p.ptrs(), C, p.count.ptr)

    def add_slab(self, slab):
        """One slab (series_stage.Slab), columns k0..k0+n-1 of the accumulators; base_x is where the slab carries se,
        base_y where it carries th."""
        with DeviceScope() as s:
            d_y = None if self.second is None else s.adopt(self.second(slab))
            x = (slab.d_ts.ptr, slab.ld, slab.se_ptr, slab.ldc, self.shift_x)
            y = x if d_y is None else (d_y.ptr, slab.n, slab.th_ptr, slab.ldc, self.shift_y)
            for p in self.passes:
                a, b = (x, y) if p is self else (y, x)
                with as_xmhw_errors(also="Unsupported"):
                    self.hl.lag_corr_accumulate(a[0], a[1], b[0], b[1], slab.isz, slab.T, slab.n, a[2], a[3], b[2], b[3],
                                                slab.D, slab.rows, a[4], b[4], self.classes, self.K, p.L, *p.ptrs(slab.k0),
                                                self.C, p.count.ptr)
            self.h.stream_sync(0)                       # the slab's series are freed on the way out

    def result(self):
        """(the six arrays over the lags lo .. hi, {n_range_x, n_range_y})"""
        self.h.stream_sync(0)
        got, counts = [p.read() for p in self.passes], [p.counts() for p in self.passes]
        # x is a partner on every step in the second pass, and in an autocorrelation: that count holds the other
        if self.second is None:
            n_range = (counts[0][1], 0)
        else:
            n_range = (counts[1][1] if len(counts) > 1 else counts[0][0], counts[0][1])
        return (assemble(got[0], got[1] if len(got) > 1 else None, self.lo, self.hi, self.second is None),
                dict(zip(self.range_texts, n_range)))


def _bytes_per_cell(T, isz, D, two):
    return (2 if two else 1) * T * isz + 2 * D * 8 + 64


def lag_corr_cells(x, y, base_x, base_y, doy, doys, classes, K, lo, hi, shift_x=0, shift_y=0, max_batch_bytes=64 << 30,
                   pad=None, counters=None, max_result_bytes=None):
    """The device stage for dense (T, C) series x and y (y None: the autocorrelation of x, nothing is uploaded twice):
    bases (Dr, C) with the labels doy (T,) / doys (Dr,) that pair steps and base rows as in detect_front.detect_cells,
    classes (T,) int labels in [-1, K), lags lo .. hi with lo <= 0 <= hi.  Returns the six arrays of FIELDS, (K, hi - lo
    + 1, C).  Cells go through the device in batches below max_batch_bytes; the sums are integers, so the batch size does
    not change a single bit.  Raises if a sample is out of range (module docstring); with ``counters`` (a dict) it
    stores ``n_range_x`` and ``n_range_y`` there instead."""
    from .device import native_float
    x = native_float(x)
    second = None
    if y is not None:
        y = np.asarray(native_float(y))
        if y.shape != np.shape(x) or y.dtype != x.dtype:
            raise XmhwException(f"x and y should be series of one shape and float type, got {x.dtype} {np.shape(x)} and "
                                f"{y.dtype} {y.shape}")

        def second(slab):
            from .device import DeviceBuffer
            d = DeviceBuffer.from_array(np.ascontiguousarray(y[:, slab.cols]))
            if pad is not None:
                pad.apply(d.ptr, slab.isz, slab.T, slab.n)
            return d
    return run_cells(_Accumulators(second, classes, K, lo, hi, shift_x, shift_y, max_result_bytes), x, base_x,
                     base_x if y is None else base_y, doy, doys, lambda T, isz, D: _bytes_per_cell(T, isz, D, y is not None),
                     max_batch_bytes, pad, counters)


def lag_corr_grid(stacked, anynans, ystacked, base_x, base_y, doy, doys, classes, K, lo, hi, shift_x=0, shift_y=0,
                  max_batch_bytes=None, clim_stacked=False, pad=None, counters=None, max_result_bytes=None):
    """lag_corr_cells() for UNCOMPACTED stacked host series (T, N): the land mask of x and its compaction run on the
    device slab by slab (series_stage.walk_grid); the slab's columns of ``ystacked`` are uploaded as they are and
    gathered on the device by the slab's mask -- the host never gathers the field.  Returns the six arrays over the ocean
    cells of x and keep[N]."""
    from .device import _gather_columns, device_itemsize, is_packed, native_float, upload_columns
    second = None
    if ystacked is not None:
        if not is_packed(ystacked):
            ystacked = np.ascontiguousarray(native_float(ystacked))
        if tuple(ystacked.shape) != tuple(stacked.shape):
            raise XmhwException(f"x and y should be series of one shape, got {tuple(stacked.shape)} and "
                                f"{tuple(ystacked.shape)}")
        if device_itemsize(ystacked) != device_itemsize(stacked if is_packed(stacked) else native_float(stacked)):
            raise XmhwException("x and y should be of one float type on the device")

        def second(slab):
            lo_, hi_, keep = slab.cols
            d_raw, isz = upload_columns(ystacked, lo_, hi_)
            if not keep.all():
                try:
                    d = _gather_columns(d_raw, isz, slab.T, hi_ - lo_, np.nonzero(keep)[0].astype(np.int64))
                finally:
                    d_raw.free()
                d_raw = d
            if pad is not None:
                pad.apply(d_raw.ptr, isz, slab.T, slab.n)
            return d_raw
    two = ystacked is not None
    isz_y = device_itemsize(ystacked) if two else 0
    # y's bytes per cell: the uploaded columns and the gathered ones
    out, keep = run_grid(_Accumulators(second, classes, K, lo, hi, shift_x, shift_y, max_result_bytes), stacked, anynans,
                         base_x, base_x if not two else base_y, doy, doys, lambda T, D: 4 * D * 8 + 64 + 2 * T * isz_y,
                         max_batch_bytes, clim_stacked, pad, counters)
    return out + (keep,)


# ---- the result --------------------------------------------------------------------------------------

def _first_true(m):
    """(index of the first True along axis 0, whether there is one)"""
    return m.argmax(axis=0), m.any(axis=0)


class LagCorrelationDataset:
    """What lag_correlation() returns, as plain arrays over (klass, lag, *spatial dims).

    klass (K,) the class labels (sorted non-negative labels found), lag (hi - lo + 1,) = lo .. hi in steps -- a positive
    lag l pairs x(t) with y(t - l): y leads --, auto: whether y was x, shift_x, shift_y.
    Raw integers: n int32 and sx, sy, sxx, syy, sxy int64 (module docstring), the sums over the valid pairs of every
    class and lag in units of 2**(shift - 16).
    Derived float64, one fixed formula on the integers, from the float64 means mx = sx / n, my = sy / n:
        mean_x   mx * 2**(shift_x - 16), mean_y likewise: the means over the PAIRS of the lag, in original units
        cov      (sxy / n - mx my) * 2**(shift_x + shift_y - 32)
        r        (sxy / n - mx my) / sqrt((sxx / n - mx**2) (syy / n - my**2)): Pearson's correlation of the pairs
        slope    (sxy / n - mx my) / (syy / n - my**2) * 2**(shift_x - shift_y): x per unit of the lagged y
    all NaN where n < 2; r and slope NaN where a variance is zero as well.
    Land: grid lines without an ocean cell are dropped, as in ClassDaysDataset; the float fields are NaN on the remaining
    land cells, integer fields are 0 there and come with the boolean ``keep`` (...) mask of the ocean cells of x."""

    def __init__(self, klass, lag, n, sx, sy, sxx, syy, sxy, keep, sdims, coords, auto=False, shift_x=0, shift_y=0,
                 tdim="time", attrs=None):
        self.klass, self.lag = np.asarray(klass), np.asarray(lag)
        self.n, self.sx, self.sy, self.sxx, self.syy, self.sxy = n, sx, sy, sxx, syy, sxy
        self.keep, self.sdims, self.coords = keep, tuple(sdims), dict(coords)
        self.auto, self.shift_x, self.shift_y = bool(auto), int(shift_x), int(shift_y)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        nf = n.astype(np.float64)
        f = lambda a: a.astype(np.float64)                                                           # noqa: E731
        few = n < 2
        with np.errstate(divide="ignore", invalid="ignore"):
            mx, my = f(sx) / nf, f(sy) / nf
            cov, vx, vy = f(sxy) / nf - mx * my, f(sxx) / nf - mx * mx, f(syy) / nf - my * my
            # a variance is zero iff n sxx == sx**2: the product wraps in 64 bits, so that is asked of a variance that
            # float64 finds negligible as well
            flat = few | ~(vx > 0.0) | ~(vy > 0.0) | self._no_spread(n, sx, sxx, vx) | self._no_spread(n, sy, syy, vy)
            self.mean_x = np.where(few, np.nan, mx * 2.0 ** (self.shift_x - BITS))
            self.mean_y = np.where(few, np.nan, my * 2.0 ** (self.shift_y - BITS))
            self.cov = np.where(few, np.nan, cov * 2.0 ** (self.shift_x + self.shift_y - 2 * BITS))
            self.r = np.where(flat, np.nan, cov / np.sqrt(vx * vy))
            self.slope = np.where(flat, np.nan, cov / vy * 2.0 ** (self.shift_x - self.shift_y))

    @staticmethod
    def _no_spread(n, s, ss, v):
        with np.errstate(over="ignore"):
            wraps = n.astype(np.uint64) * ss.astype(np.uint64) == s.astype(np.uint64) * s.astype(np.uint64)
        return wraps & (np.abs(v) <= 2.0 ** -40 * (ss.astype(np.float64) / np.maximum(n, 1)))

    def _at(self, lag):
        i = np.nonzero(self.lag == lag)[0]
        if not i.size:
            raise XmhwException(f"lag {lag} is not among the lags {int(self.lag[0])} .. {int(self.lag[-1])}")
        return int(i[0])

    def lag_of_max(self):
        """(lag, r): per class and cell the lag of the largest |r| (the first of equals) and that r, both float64 over
        (klass, *spatial dims), NaN where no lag has a correlation"""
        a = np.where(np.isnan(self.r), -1.0, np.abs(self.r))
        i = a.argmax(axis=1)
        r = np.take_along_axis(self.r, i[:, None], axis=1)[:, 0]
        return np.where(np.isnan(r), np.nan, self.lag[i].astype(np.float64)), r

    def _acf(self, who):
        """r over the lags 0 .. hi as (lag, klass, ...)"""
        if not self.auto:
            raise XmhwException(f"{who} is defined for an autocorrelation (y=None) only")
        return np.moveaxis(self.r[:, self._at(0):], 1, 0)

    def efolding_time(self):
        """The e-folding (decorrelation) time in steps, (klass, *spatial dims): the first lag at which r < 1 / e, linearly
        interpolated between it and the lag before; +inf if r stays at or above 1 / e up to the largest lag; NaN where
        the autocorrelation is undefined.  An autocorrelation only."""
        r = self._acf("efolding_time")
        e = math.exp(-1.0)
        below = r < e
        below[0] = False
        i, some = _first_true(below)
        i1 = np.maximum(i, 1)
        hi_ = np.take_along_axis(r, (i1 - 1)[None], axis=0)[0]
        lo_ = np.take_along_axis(r, i1[None], axis=0)[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (i1 - 1) + (hi_ - e) / (hi_ - lo_)
        out = np.where(some, t, np.inf)
        return np.where(np.isnan(r[0]), np.nan, out)

    def integral_time_scale(self):
        """1 + 2 sum of r over the lags 1 .. m - 1, m the first lag with r <= 0 (all the lags if there is none), in steps,
        (klass, *spatial dims); NaN where the autocorrelation is undefined.  An autocorrelation only."""
        r = self._acf("integral_time_scale")
        stop = r <= 0.0
        stop[0] = False
        i, some = _first_true(stop)
        m = np.where(some, i, r.shape[0])
        lags = np.arange(r.shape[0]).reshape((-1,) + (1,) * (r.ndim - 1))
        used = (lags >= 1) & (lags < m[None])
        return 1.0 + 2.0 * np.where(used, r, 0.0).sum(axis=0) + np.where(np.isnan(r[0]), np.nan, 0.0)

    def n_eff(self):
        """The effective sample size n_0 / integral_time_scale(), clipped to [2, n_0], n_0 the pairs at lag 0; (klass,
        *spatial dims).  An autocorrelation only."""
        tint = self.integral_time_scale()
        n0 = self.n[:, self._at(0)].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.minimum(np.maximum(n0 / tint, 2.0), n0)
        return np.where(np.isnan(tint), np.nan, out)

    def p_value(self, n_eff=None):
        """Two-sided p-value of r, Student's t with n_eff - 2 degrees of freedom of r sqrt((n_eff - 2) / (1 - r**2)), over
        (klass, lag, *spatial dims); NaN where n_eff <= 2.  ``n_eff``: an array that broadcasts against
        (klass, *spatial dims); or the pair (autocorrelation dataset of x, of y), both with lag 1, for Bretherton's
        n (1 - r1x r1y) / (1 + r1x r1y) clipped to [2, n] with n the pairs of every lag; None: this dataset's own n_eff(),
        for an autocorrelation only."""
        nf = self.n.astype(np.float64)
        if n_eff is None:
            if not self.auto:
                raise XmhwException("p_value of two fields needs n_eff: an array, or the two autocorrelation datasets")
            ne = self.n_eff()[:, None]
        elif isinstance(n_eff, (tuple, list)) and len(n_eff) == 2 and all(isinstance(d, LagCorrelationDataset) for d in n_eff):
            if not all(d.auto for d in n_eff):
                raise XmhwException("p_value takes the AUTOcorrelation datasets of the two fields")
            rr = (n_eff[0].r[:, n_eff[0]._at(1)] * n_eff[1].r[:, n_eff[1]._at(1)])[:, None]
            with np.errstate(invalid="ignore", divide="ignore"):
                ne = np.minimum(np.maximum(nf * (1.0 - rr) / (1.0 + rr), 2.0), nf)
        else:
            ne = np.asarray(n_eff, dtype=np.float64)
            ne = ne[:, None] if ne.ndim == self.r.ndim - 1 else ne
        with np.errstate(divide="ignore", invalid="ignore"):
            dof = np.broadcast_to(ne - 2.0, self.r.shape)
            t = self.r * np.sqrt(dof / (1.0 - self.r * self.r))
            return p_two_sided(t, dof)

    def to_xarray(self):
        import xarray as xr
        cell = ("klass", "lag") + self.sdims
        data = {k: (cell, getattr(self, k)) for k in FIELDS + ("mean_x", "mean_y", "cov", "r", "slope")}
        data.update(keep=(self.sdims, self.keep))
        return xr.Dataset(data, coords=dict({"klass": self.klass, "lag": self.lag},
                                            **{d: self.coords[d] for d in self.sdims if d in self.coords}),
                          attrs=dict(self.attrs, auto=int(self.auto), shift_x=self.shift_x, shift_y=self.shift_y))


# ---- the public function -----------------------------------------------------------------------------

def _base_on_ocean(base, ocean, point, sdims, sshape, coords, name):
    """``base`` as the ('doy', ...) GridSeries that pairs with the ocean cells of x as a climatology does: None is zero;
    NaN on the land of x and, where the base itself is missing on an ocean cell of x (a cell that is land in y), zero --
    the samples there are NaN anyway"""
    if base is None:
        return zero_base(ocean, point, sdims, sshape, coords)
    base = base_series(base, point, sdims, coords)
    if point:
        return base
    v = np.asarray(base.values, dtype=np.float64)
    order = [base.dims.index("doy")] + [base.dims.index(d) for d in sdims]
    v = np.transpose(v, order)
    if v.shape[1:] != tuple(sshape):
        raise XmhwException(f"{name} should be on the grid of x {tuple(sshape)}, got {v.shape[1:]}")
    sea = ocean.reshape(sshape)
    v = np.where(sea, np.where(np.isnan(v), 0.0, v), np.nan)
    return GridSeries(v, ("doy",) + tuple(sdims), dict(base.coords))


def lag_correlation(x, y=None, base_x=None, base_y=None, lags=(0, 30), classes="all", shift_x=0, shift_y=0, tdim="time",
                    maxPadLength=None, anynans=False, max_batch_bytes=None, max_result_bytes=8 << 30, _compute=None):
    """Lagged correlation per cell: for every class of time steps and every lag l in ``lags`` = (lo, hi), the sums
    behind the correlation of ``x - base_x`` at step t with ``y - base_y`` at step t - l.

    ``x``, ``base_x`` and ``classes`` are taken as index_regression() takes ``temp``, ``base`` and ``classes``: land
    masking, padding, a constant base per cell or a ('doy', ...) climatology on the grid of ``x``, at most 64 classes;
    a base of None is zero.  ``y=None`` is the autocorrelation of ``x`` (``base_y`` and ``shift_y`` are then those of
    x); a given ``y`` is a series on the same grid and time axis, padded like ``x``; fields of different float types are
    both taken as float64, and a one-row base beside a many-row base is repeated to its rows.  The cells are those that
    are ocean in ``x``; a cell that is all-NaN in ``y`` has n = 0.
    ``lags``: lo <= 0 <= hi, at most 63 steps either way.  A POSITIVE lag l means that y LEADS x by l steps (x(t) with
    y(t - l)), a negative lag that x leads.  The class of a pair is that of its LATER step, at positive and at negative
    lags alike; the earlier step may be of any class.  Negative lags of two fields take a second device pass with the
    roles of the fields exchanged; lag 0 comes from the first.
    ``shift_x``, ``shift_y``: samples enter as (field - base) * 2**-shift and must then lie inside (-2**7, 2**7).  The
    (klass, lag, cells) accumulators take 44 bytes an entry: the call raises if that exceeds ``max_result_bytes``.

    Returns a LagCorrelationDataset.  Raises if a sample is out of range.  ``_compute``: a stand-in for lag_corr_cells()
    (host tests)."""
    from .landmask import stack_cells
    lo, hi = check_lags(lags)
    shift_x, shift_y = check_shifts(shift_x, shift_y)
    auto = y is None
    if auto:
        if base_y is not None:
            raise XmhwException("base_y belongs to y: an autocorrelation (y=None) takes base_x alone")
        shift_y = shift_x
    layout = grid_layout(x, tdim)
    coords, _, dims, point, sdims, sshape, N = layout
    time = np.asarray(coords[tdim])
    T = time.shape[0]
    check_steps(T, "lag_correlation")
    ydims = None
    if not auto:
        ycoords, _, ydims, ypoint, ysdims, ysshape, _ = grid_layout(y, tdim)
        check_same_frame("lag_correlation", "x", "y", (point, sdims, sshape), time, (ypoint, ysdims, ysshape), ycoords[tdim])
        xv, yv = np.asarray(x.values), np.asarray(y.values)
        if xv.dtype != yv.dtype or xv.dtype.kind != "f":
            # one float type on the device: float64 holds both
            as64 = lambda g, v, d: GridSeries(v.astype(np.float64), tuple(d),                        # noqa: E731
                                              _from_xarray(g)[0] if _is_xarray(g) else dict(g.coords))
            x, y = as64(x, xv, dims), as64(y, yv, ydims)
            layout = grid_layout(x, tdim)
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "lag_correlation", "classes")
    ocean = ocean_mask(x, dims, tdim, point, anynans)
    bx = _base_on_ocean(base_x, ocean, point, sdims, sshape, coords, "base_x")
    by = bx if auto else _base_on_ocean(base_y, ocean, point, sdims, sshape, coords, "base_y")
    if not auto:
        rx, ry = np.asarray(bx.values).shape[bx.dims.index("doy")], np.asarray(by.values).shape[by.dims.index("doy")]
        if rx != ry and 1 in (rx, ry):
            # a one-row base beside a many-row base: repeated to its rows
            one, many = (bx, by) if rx == 1 else (by, bx)
            v = np.repeat(np.moveaxis(np.asarray(one.values), one.dims.index("doy"), 0), max(rx, ry), axis=0)
            rep = GridSeries(v, ("doy",) + tuple(d for d in one.dims if d != "doy"),
                             dict(one.coords, doy=np.asarray(many.coords["doy"])))
            bx, by = (rep, by) if rx == 1 else (bx, rep)
        elif rx != ry:
            raise XmhwException(f"base_x and base_y have {rx} and {ry} rows")
    ystack = None
    if not auto:
        ystack = (np.asarray(y.values).reshape(-1, 1) if point else stack_cells(np.asarray(y.values), ydims, tdim)[0])
    more = (kid, K, lo, hi, shift_x, shift_y)

    def on_cells(host_keep, ts, sec, thc, doy, doys, options, **extra):
        check_result_bytes(K, lo, hi, ts.shape[1], max_result_bytes)
        ycells = None if auto else (ystack if point else ystack[:, host_keep()])
        return (_compute or lag_corr_cells)(ts, ycells, sec, None if auto else thc, doy, doys, *more,
                                            max_result_bytes=max_result_bytes, **extra)

    f, arrays, mhw = cell_stage(
        "lag correlation", x, by, bx, layout, tdim, on_cells,
        lambda stacked, anynans_, sec, thc, doy, doys, options, **extra:
            lag_corr_grid(stacked, anynans_, ystack, sec, None if auto else thc, doy, doys, *more,
                          max_result_bytes=max_result_bytes, **extra),
        lambda C: [(K, hi - lo + 1, C)] * 6, _range_texts(shift_x, shift_y), maxPadLength=maxPadLength, anynans=anynans,
        _compute=_compute, max_batch_bytes=max_batch_bytes)
    raw = [f.place(a, 0, np.int32 if k == "n" else np.int64) for k, a in zip(FIELDS, arrays)]
    out = LagCorrelationDataset(class_result_labels(found), np.arange(lo, hi + 1), *raw, f.keep, f.sdims, f.coords, auto,
                                shift_x, shift_y, tdim, stage_attrs(classes, mhw))
    land = ~np.asarray(out.keep, dtype=bool)
    if not point:
        for a in (out.mean_x, out.mean_y, out.cov, out.r, out.slope):
            a[..., land] = np.nan
    return out
