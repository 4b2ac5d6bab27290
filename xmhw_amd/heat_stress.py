"""heat_stress(): accumulated thermal stress -- how much heat has piled up in a cell over the last W steps -- and its
baseline, maximum_monthly_mean().  With W = 84 daily steps, a hot-spot floor of 1 degree above the Maximum Monthly Mean
and weeks as the unit this is the Degree Heating Week (DHW) of NOAA Coral Reef Watch (Liu et al. 2014; Skirving et al.
2020), the operational heat-stress index that MHW studies set beside the Hobday categories.  It cannot come from the
event table (events, not a trailing window) nor from mhw_days_by() (in-event steps only): it is one more streaming pass
over the series, and the first stage with a window along time (csrc/kernels_stress.hip).

Class sums of the series (for the MMM).  ``class_of_t``: one int32 label per step in [-1, K), -1 = the step counts
nowhere; ``x0`` a scalar.  Per class k and cell c, over the steps of class k, with d = float64(sample) - x0:
    n_valid[k, c] (int32)   steps whose d is not NaN and |d| < 2**7
    sum_q[k, c]   (int64)   sum of rint(d * 2**16) over those steps
Any other non-NaN d is left out and counted in n_range; maximum_monthly_mean() raises if n_range > 0.  The monthly mean
is x0 + sum_q / n_valid / 2**16 in float64, the MMM its maximum over the 12 calendar months, NaN where a month has no
valid step.

Heat stress.  ``base`` (D, C) float64 with the base row of every step: D = 1 is a constant per cell such as the MMM,
D = 366 is ``seas`` or ``thresh`` of threshold().  With x = float64(sample) and b = base[row(t), c], both negated under
coldSpells, and h = x - b:
    the step is hot iff h == h, h >= h0 and h < 2**7                  (2**-16 <= h0 < 2**7)
    q(t) = int64(rint(h * 2**16)) on hot steps, 0 otherwise
    S(t) = sum of q(i) over max(0, t - W + 1) <= i <= t               (1 <= W <= 255, so S < 2**31)
A step with h >= 2**7 or infinite is not hot and is counted in n_range (heat_stress() raises if n_range > 0).  A step
of class -1 feeds the window of later steps but is reduced nowhere.  Per class k and cell c, over the steps of class k:
    counts[k, 0, c]     (int32)   steps with h not NaN
    counts[k, 1, c]     (int32)   hot steps
    counts[k, 2 + l, c] (int32)   steps with S(t) >= level_q[l], l < L <= 6 (the channels 2 + L .. 7 stay 0)
    hsum_q[k, c]        (int64)   sum of q(t): the degree heating days of the class
    peak_q[k, c]        (int32)   max S(t)
    peak_t[k, c]        (int32)   the smallest t that attains peak_q (a class without steps: peak_q = 0, peak_t = -1)
    snap_q[j, c]        (int32)   S(at[j]) for the J <= 64 snapshot steps, whatever the class of that step
Units: level_q = rint(level * unit * 2**16) and DHW = S / (unit * 2**16).  Everything is an integer sum or an integer
maximum: the result does not depend on the time blocks, the slabs, the launch geometry or the schedule.

Host side here (validation, class labels, baseline, slabs, land); device side in csrc/kernels_stress.hip behind
heat_stress_cells() / class_sums_cells() (a compact host series) and heat_stress_grid() / class_sums_grid() (a stacked
grid, masked and compacted on the device slab by slab).  The baseline rides where the walkers carry the climatologies.
"""
import numpy as np

from . import calendar as cal
from ._lib import hip_stress
from .api import GridSeries
from .device import as_xmhw_errors
from .exception import XmhwException
from .series_stage import (Accumulators, base_series, cell_stage, check_class_ids, class_labels, class_result_labels,
                           dense_ids, grid_layout, ocean_mask, run_cells, run_grid, stage_attrs, zero_base)

MAX_CLASSES = 1024              # XMHW_HEAT_STRESS_MAX_CLASSES (include/xmhw_amd.h)
CHANNELS = 8                    # XMHW_HEAT_STRESS_CHANNELS: n_valid, n_hot, then the levels
MAX_LEVELS = 6                  # XMHW_HEAT_STRESS_MAX_LEVELS
MAX_SNAPSHOTS = 64              # XMHW_HEAT_STRESS_MAX_SNAPSHOTS
MAX_WINDOW = 255                # XMHW_HEAT_STRESS_MAX_WINDOW
BITS = 16                       # XMHW_HEAT_STRESS_BITS
RANGE_BITS = 7                  # h < 2**7, |d| < 2**7
_ONE = float(1 << BITS)
_RANGE_TEXT = ("samples lie 2**7 and more above their baseline (or are infinite): is the series in kelvin and the "
               "baseline in degrees Celsius?")
_SUMS_RANGE_TEXT = ("samples lie 2**7 and more from offset (or are infinite): for a series in kelvin pass "
                    "offset=273.15")


# ---- validation (mirrors the refusals of the C entries) ----------------------------------------------

def check_stress_arguments(T, classes, K, window, h0, level_q, at):
    """The stage-side check: (classes int32 (T,), K, W, h0, level_q int64 (L,), at int32 (J,))"""
    classes, K = check_class_ids(T, classes, K, MAX_CLASSES, "heat_stress")
    if int(window) != window or not 1 <= int(window) <= MAX_WINDOW:
        raise XmhwException(f"window should be a whole number of steps in [1, {MAX_WINDOW}], got {window!r}")
    h0 = float(h0)
    if not (2.0 ** -BITS <= h0 < 2.0 ** RANGE_BITS):
        raise XmhwException(f"the hot-spot floor should be in [2**-{BITS}, 2**{RANGE_BITS}), got {h0!r}")
    level_q = np.asarray(level_q)
    if level_q.ndim != 1 or (level_q.size and level_q.dtype.kind not in "iu"):
        raise XmhwException("level_q should be a 1-D integer array")
    if level_q.shape[0] > MAX_LEVELS:
        raise XmhwException(f"heat_stress handles at most {MAX_LEVELS} levels, got {level_q.shape[0]}")
    level_q = np.ascontiguousarray(level_q, dtype=np.int64)
    if (np.diff(level_q) <= 0).any():
        raise XmhwException("levels should be strictly ascending")
    at = np.asarray(at)
    if at.ndim != 1 or (at.size and at.dtype.kind not in "iu"):
        raise XmhwException("at should be a 1-D array of time steps")
    if at.shape[0] > MAX_SNAPSHOTS:
        raise XmhwException(f"heat_stress handles at most {MAX_SNAPSHOTS} snapshot steps, got {at.shape[0]}")
    at = at.astype(np.int64)
    if at.size and (at.min() < 0 or at.max() >= T):
        raise XmhwException(f"snapshot steps should be in [0, {T})")
    if (np.diff(at) <= 0).any():
        raise XmhwException("snapshot steps should be strictly ascending")
    return classes, K, int(window), h0, level_q, np.ascontiguousarray(at, dtype=np.int32)


def levels_q(levels, unit):
    """level_q = rint(level * unit * 2**16) of the levels given in units of ``unit`` steps (weeks: unit = 7 days)"""
    unit = float(unit)
    if not (np.isfinite(unit) and unit > 0.0):
        raise XmhwException(f"unit should be a positive number of steps, got {unit!r}")
    levels = np.atleast_1d(np.asarray(levels if levels is not None else (), dtype=np.float64))
    if levels.ndim != 1 or not np.isfinite(levels).all():
        raise XmhwException("levels should be a sequence of finite numbers")
    if levels.shape[0] > MAX_LEVELS:
        raise XmhwException(f"heat_stress handles at most {MAX_LEVELS} levels, got {levels.shape[0]}")
    if (np.abs(levels * unit) >= 2.0 ** 40).any():
        raise XmhwException("levels are out of range")
    return np.rint(levels * unit * _ONE).astype(np.int64)


def snapshot_steps(at, time):
    """``at`` as time steps: integers as they are, datetime64 values looked up on the time axis"""
    if at is None:
        return np.zeros(0, dtype=np.int64)
    at = np.atleast_1d(np.asarray(at))
    if at.ndim != 1:
        raise XmhwException("at should be a list of time steps or datetime64 values")
    if at.size == 0:
        return np.zeros(0, dtype=np.int64)
    if at.dtype.kind in "US":                               # "2016-03-15"
        try:
            at = at.astype("datetime64[D]")
        except ValueError as e:
            raise XmhwException(f"at holds a string that is not a date: {e}") from e
    if at.dtype.kind == "M":
        time = np.asarray(time)
        if time.dtype.kind != "M":
            raise XmhwException(f"datetime64 snapshot steps need a datetime64 time coordinate, got {time.dtype}")
        days = time.astype("datetime64[D]")
        pos = np.searchsorted(days, at.astype("datetime64[D]"))
        ok = pos < days.shape[0]
        if not ok.all() or (days[np.minimum(pos, days.shape[0] - 1)] != at.astype("datetime64[D]")).any():
            raise XmhwException("a snapshot date is not on the time axis")
        return pos.astype(np.int64)
    if at.dtype.kind not in "iu":
        raise XmhwException(f"at should hold time steps (integers) or datetime64 values, got {at.dtype}")
    return at.astype(np.int64)


# ---- the device stages -------------------------------------------------------------------------------

class _StressAccumulators(Accumulators):
    """One call's arguments and its device accumulators: counts int32 (K, 8, C), hsum_q int64 (K, C), the peak keys
    (K, C), snap_q int32 (J, C) and the range counter; peak_q and peak_t are what finish() makes of the keys."""
    range_texts = {"n_range": _RANGE_TEXT}
    _ADDED = ("counts", "hsum_q", "key", "snap_q")

    def __init__(self, classes, K, window, h0, level_q, at, coldSpells):
        super().__init__()
        self.hs = hip_stress()
        self.args = (classes, K, window, h0, level_q, at)
        self.neg = int(bool(coldSpells))

    def begin(self, T, C):
        """T steps, C ocean cells"""
        self.classes, self.K, self.W, self.h0, self.level_q, self.at = check_stress_arguments(T, *self.args)
        K, J = self.K, int(self.at.shape[0])
        self.make(C, {"counts": ((K, CHANNELS, C), np.int32), "hsum_q": ((K, C), np.int64), "key": ((K, C), np.int64),
                      "peak_q": ((K, C), np.int32), "peak_t": ((K, C), np.int32), "snap_q": ((J, C), np.int32)})
        with as_xmhw_errors(also="Unsupported"):
            self.hs.heat_stress_init(K, C, *self.ptrs(0, self._ADDED[:3]), C, self.count.ptr)

    def add_slab(self, slab):
        """One slab (series_stage.Slab), columns k0..k0+n-1 of the accumulators; the baseline is where the slab carries
        its climatologies."""
        with as_xmhw_errors(also="Unsupported"):
            self.hs.heat_stress_accumulate(slab.d_ts.ptr, slab.isz, slab.T, slab.n, slab.ld, slab.se_ptr, slab.ldc, slab.D,
                                           slab.rows, self.neg, self.W, self.h0, self.classes, self.K, self.level_q, self.at,
                                           *self.ptrs(slab.k0, self._ADDED), self.C, self.count.ptr)
        self.h.stream_sync(0)                           # the slab's series is freed on the way out

    def finish(self):
        with as_xmhw_errors(also="Unsupported"):
            self.hs.heat_stress_finish(self.K, self.C, *self.ptrs(0, ("key", "peak_q", "peak_t")), self.C)

    def read(self):
        return super().read(("counts", "hsum_q", "peak_q", "peak_t", "snap_q"))


class _SumsAccumulators(Accumulators):
    """The class sums' counterpart: n_valid int32 (K, C), sum_q int64 (K, C) and the range counter."""
    range_texts = {"n_range": _SUMS_RANGE_TEXT}

    def __init__(self, classes, K, x0):
        super().__init__()
        self.hs = hip_stress()
        self.classes, self.K = classes, K
        self.x0 = float(x0)
        if not np.isfinite(self.x0):
            raise XmhwException(f"offset should be finite, got {x0!r}")

    def begin(self, T, C):
        self.classes, self.K = check_class_ids(T, self.classes, self.K, MAX_CLASSES, "class_sums")
        self.make(C, {"n_valid": ((self.K, C), np.int32), "sum_q": ((self.K, C), np.int64)})
        with as_xmhw_errors(also="Unsupported"):
            self.hs.class_sums_init(self.K, C, *self.ptrs(), C, self.count.ptr)

    def add_slab(self, slab):
        with as_xmhw_errors(also="Unsupported"):
            self.hs.class_sums_accumulate(slab.d_ts.ptr, slab.isz, slab.T, slab.n, slab.ld, self.x0, self.classes, self.K,
                                          *self.ptrs(slab.k0), self.C, self.count.ptr)
        self.h.stream_sync(0)


def _bytes_per_cell(T, isz, D):
    return T * isz + 2 * D * 8 + 64


def _extra_per_cell(T, D):
    return 4 * D * 8 + 64


def heat_stress_cells(ts, base, doy, doys, classes, K, window, h0, level_q, at, coldSpells=False, max_batch_bytes=64 << 30,
                      pad=None, counters=None):
    """The device stage for a dense (T, C) series: base (D, C) with the labels doy (T,) / doys (D,) that pair steps and
    base rows as in detect_front.detect_cells, classes (T,) int labels in [-1, K), level_q int64 (L,), at int (J,).
    Returns (counts int32 (K, 8, C), hsum_q int64 (K, C), peak_q int32 (K, C), peak_t int32 (K, C), snap_q int32 (J, C)).
    Cells go through the device in batches below max_batch_bytes; the sums are integers, so the batch size does not
    change a single bit.  Raises if a sample is out of range (module docstring); with ``counters`` (a dict) it stores
    ``n_range`` there instead."""
    return run_cells(_StressAccumulators(classes, K, window, h0, level_q, at, coldSpells), ts, base, base, doy, doys,
                     _bytes_per_cell, max_batch_bytes, pad, counters)


def heat_stress_grid(stacked, anynans, base, doy, doys, classes, K, window, h0, level_q, at, coldSpells=False,
                     max_batch_bytes=None, clim_stacked=False, pad=None, counters=None):
    """heat_stress_cells() for an UNCOMPACTED stacked host series (T, N), float or a packed int16 view: the land mask
    and the compaction run on the device slab by slab (series_stage.walk_grid).  Returns the five arrays over the ocean
    cells and keep[N]."""
    out, keep = run_grid(_StressAccumulators(classes, K, window, h0, level_q, at, coldSpells), stacked, anynans, base, base,
                         doy, doys, _extra_per_cell, max_batch_bytes, clim_stacked, pad, counters)
    return out + (keep,)


def class_sums_cells(ts, classes, K, x0=0.0, max_batch_bytes=64 << 30, pad=None, counters=None):
    """The class sums of a dense (T, C) series: (n_valid int32 (K, C), sum_q int64 (K, C))"""
    ts = np.asarray(ts)
    zero, steps = np.zeros((1, ts.shape[1])), np.zeros(ts.shape[0], dtype=np.int64)
    return run_cells(_SumsAccumulators(classes, K, x0), ts, zero, zero, steps, steps[:1], _bytes_per_cell, max_batch_bytes,
                     pad, counters)


def class_sums_grid(stacked, anynans, land, classes, K, x0=0.0, max_batch_bytes=None, clim_stacked=False, pad=None,
                    counters=None):
    """class_sums_cells() for an uncompacted stacked series (T, N); ``land`` (1, N) is NaN on the land cells and pairs
    the slabs' survivors with the accumulators' columns, as the climatologies do elsewhere.  Returns (n_valid, sum_q,
    keep[N])."""
    steps = np.zeros(stacked.shape[0], dtype=np.int64)
    out, keep = run_grid(_SumsAccumulators(classes, K, x0), stacked, anynans, land, land, steps, steps[:1], _extra_per_cell,
                         max_batch_bytes, clim_stacked, pad, counters)
    return out + (keep,)


# ---- results -----------------------------------------------------------------------------------------

class MonthlyMeanDataset:
    """What maximum_monthly_mean() returns: mmm float64 (...), monthly_mean float64 (12, ...), n_valid int32 (12, ...),
    sum_q int64 (12, ...), keep (...) over the spatial dims; ``offset`` the x0 of the sums.  NaN on land and where a
    month has no valid step.  heat_stress() takes it as ``base``."""

    def __init__(self, n_valid, sum_q, keep, sdims, coords, offset, period, attrs=None):
        self.n_valid, self.sum_q, self.keep = n_valid, sum_q, keep
        self.sdims, self.coords, self.offset, self.period = tuple(sdims), dict(coords), float(offset), period
        self.attrs = dict(attrs or {})
        self.month = np.arange(1, 13)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.monthly_mean = self.offset + sum_q.astype(np.float64) / n_valid.astype(np.float64) / _ONE
        self.monthly_mean[n_valid == 0] = np.nan
        self.mmm = self.monthly_mean.max(axis=0)                     # NaN where a month is NaN

    def as_series(self):
        """the MMM as the GridSeries that heat_stress() pairs with the series"""
        return GridSeries(self.mmm, self.sdims, self.coords)

    def to_xarray(self):
        import xarray as xr
        return xr.Dataset({"mmm": (self.sdims, self.mmm), "monthly_mean": (("month",) + self.sdims, self.monthly_mean),
                           "n_valid": (("month",) + self.sdims, self.n_valid), "keep": (self.sdims, self.keep)},
                          coords=dict({"month": self.month}, **{d: self.coords[d] for d in self.sdims}), attrs=self.attrs)


class HeatStressDataset:
    """What heat_stress() returns, as plain arrays over (klass, *spatial dims) unless noted.

    klass (K,) the class labels (sorted non-negative labels found), n_steps (K,) the time steps of each class;
    n_valid, n_hot int32; n_level int32 (K, L, ...): steps at or above each of ``levels``; hsum_q int64; peak_q, peak_t
    int32 (peak_t = -1: no step); snap_q int32 (J, ...) at the time steps ``at`` (J,), ``time_at`` their time labels.
    Derived float64 views: dhw_peak = peak_q / (unit * 2**16), dhw_at = snap_q / (unit * 2**16) (in ``unit`` steps x
    degrees: degree heating weeks for unit = 7 days), degree_days = hsum_q / 2**16.
    Land: grid lines without an ocean cell are dropped, as in ClassDaysDataset; the float views are NaN on the remaining
    land cells, integer fields are 0 there (peak_t -1) and come with the boolean ``keep`` (...) mask of the ocean cells."""

    def __init__(self, klass, n_steps, n_valid, n_hot, n_level, hsum_q, peak_q, peak_t, snap_q, at, time_at, keep, sdims,
                 coords, window, unit, levels, tdim="time", attrs=None):
        self.klass, self.n_steps = np.asarray(klass), np.asarray(n_steps)
        self.n_valid, self.n_hot, self.n_level, self.hsum_q = n_valid, n_hot, n_level, hsum_q
        self.peak_q, self.peak_t, self.snap_q = peak_q, peak_t, snap_q
        self.at, self.time_at = np.asarray(at), np.asarray(time_at)
        self.keep, self.sdims, self.coords = keep, tuple(sdims), dict(coords)
        self.window, self.unit, self.levels = int(window), float(unit), np.asarray(levels, dtype=np.float64)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        scale = self.unit * _ONE
        self.dhw_peak = peak_q.astype(np.float64) / scale
        self.dhw_at = snap_q.astype(np.float64) / scale
        self.degree_days = hsum_q.astype(np.float64) / _ONE
        for a in (self.dhw_peak, self.dhw_at, self.degree_days):
            a[..., ~np.asarray(keep, dtype=bool)] = np.nan

    def quantisation_bound(self):
        """Bound on |dhw - the float64 sum of the hot h of the window / unit| from the fixed point alone: every
        rint(h * 2**16) / 2**16 is within 2**-17 of its h (the product by 2**16 is exact), so S / 2**16 is within
        W * 2**-17 of the exact window sum.  S < 2**31 converts to float64 exactly, unit * 2**16 rounds by 2**-53
        relative and the division by half an ulp more: on a value below 2**15 / unit that is less than 2**-37 / unit."""
        return (self.window * 2.0 ** -17 + 2.0 ** -37) / self.unit

    def to_xarray(self):
        import xarray as xr
        cell = ("klass",) + self.sdims
        return xr.Dataset(
            {"n_valid": (cell, self.n_valid), "n_hot": (cell, self.n_hot), "n_level": (("klass", "level") + self.sdims, self.n_level),
             "hsum_q": (cell, self.hsum_q), "peak_q": (cell, self.peak_q), "peak_t": (cell, self.peak_t),
             "snap_q": (("at",) + self.sdims, self.snap_q), "dhw_peak": (cell, self.dhw_peak),
             "dhw_at": (("at",) + self.sdims, self.dhw_at), "degree_days": (cell, self.degree_days),
             "n_steps": (("klass",), self.n_steps), "keep": (self.sdims, self.keep)},
            coords=dict({"klass": self.klass, "level": self.levels, "at": self.time_at},
                        **{d: self.coords[d] for d in self.sdims}), attrs=self.attrs)


# ---- the public functions ----------------------------------------------------------------------------

def heat_stress(temp, base, window=84, min_hotspot=1.0, unit=7.0, levels=(4.0, 8.0), classes="year", at=None, tdim="time",
                coldSpells=False, maxPadLength=None, tstep=False, anynans=False, max_batch_bytes=None, _compute=None):
    """Accumulated thermal stress per cell: the sum over the last ``window`` steps of the excess of ``temp`` over
    ``base`` on the steps where it reaches ``min_hotspot``; reduced per class of time steps, and snapshots of it.

    ``temp`` and the options shared with detect() mean and validate what they do there (land masking, padding, cold
    spells: both series and base negated).  ``base``: a spatial array / GridSeries / DataArray on the grid of ``temp``
    (a constant per cell, e.g. the MonthlyMeanDataset of maximum_monthly_mean(), which is taken as it is), or a
    ('doy', ...) climatology as threshold() returns (climatology_series()); its cells pair with the series' ocean cells
    by position, as th and se do.  ``unit``: the steps in one unit of the result (7 daily steps: weeks); ``levels``: up to
    6 ascending levels in those units (Coral Reef Watch: 4 and 8 degree heating weeks, Alert Level 1 and 2).
    ``classes``: as in mhw_days_by().  ``at``: up to 64 ascending time steps or datetime64 values for which the whole
    map of S is returned.

    Returns a HeatStressDataset.  Raises if a sample lies 2**7 and more above its baseline.  ``_compute``: a stand-in
    for heat_stress_cells() (host tests)."""
    layout = grid_layout(temp, tdim)
    coords, _, _, point, sdims, sshape, N = layout
    time = np.asarray(coords[tdim])
    T = time.shape[0]
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "heat_stress", "classes")
    level_q = levels_q(levels, unit)
    kid, K, window, h0, level_q, steps = check_stress_arguments(T, kid, K, window, min_hotspot, level_q,
                                                                snapshot_steps(at, time))
    n_steps = np.bincount(kid[kid >= 0], minlength=K).astype(np.int64)
    base = base_series(base, point, sdims, coords)
    J, L = steps.shape[0], level_q.shape[0]
    more = (kid, K, window, h0, level_q, steps)
    f, (counts, hsum, pq, pt, snap), mhw = cell_stage(
        "stress", temp, base, base, layout, tdim,
        lambda host_keep, ts, sec, thc, doy, doys, options, **extra:
            (_compute or heat_stress_cells)(ts, sec, doy, doys, *more, coldSpells=options[3], **extra),
        lambda stacked, anynans_, sec, thc, doy, doys, options, **extra:
            heat_stress_grid(stacked, anynans_, sec, doy, doys, *more, coldSpells=options[3], **extra),
        lambda C: ((K, CHANNELS, C), (K, C), (K, C), (K, C), (J, C)), _StressAccumulators.range_texts,
        maxPadLength=maxPadLength, coldSpells=coldSpells, tstep=tstep, anynans=anynans, _compute=_compute,
        max_batch_bytes=max_batch_bytes)
    attrs = stage_attrs(classes, mhw, window=window, min_hotspot=h0, unit=float(unit))
    return HeatStressDataset(class_result_labels(found), n_steps, f.place(counts[:, 0], 0, np.int32),
                             f.place(counts[:, 1], 0, np.int32), f.place(counts[:, 2:2 + L], 0, np.int32), f.place(hsum, 0, np.int64), f.place(pq, 0, np.int32),
                             f.place(pt, -1, np.int32), f.place(snap, 0, np.int32), steps, time[steps], f.keep, f.sdims,
                             f.coords, window, unit, np.atleast_1d(np.asarray(levels if levels is not None else (),
                                                                              dtype=np.float64)), tdim, attrs)


def _period_labels(time, period):
    """month - 1 of every step inside ``period`` (None: all steps; (first, last) calendar years or datetime64 values,
    both inclusive), -1 outside"""
    if time.dtype.kind != "M":
        raise XmhwException(f"maximum_monthly_mean needs a datetime64 time coordinate, got {time.dtype}")
    year, month, _, _ = cal._fields(time)
    inside = np.ones(time.shape[0], dtype=bool)
    if period is not None:
        if len(period) != 2:
            raise XmhwException("period should be (first, last): calendar years or datetime64 values, both inclusive")
        lo, hi = (np.asarray(p) for p in period)
        if lo.dtype.kind == "M" or hi.dtype.kind == "M" or lo.dtype.kind in "US":
            days = time.astype("datetime64[D]")
            inside = (days >= lo.astype("datetime64[D]")) & (days <= hi.astype("datetime64[D]"))
        else:
            inside = (year >= int(lo)) & (year <= int(hi))
    if not inside.any():
        raise XmhwException(f"period {period!r} selects no time step")
    return np.where(inside, month - 1, -1).astype(np.int32)


def maximum_monthly_mean(temp, period=None, tdim="time", offset=0.0, anynans=False, max_batch_bytes=None, _compute=None):
    """The Maximum Monthly Mean of Coral Reef Watch: per cell, the largest of the 12 calendar-month means of ``temp``
    over ``period`` (None: the whole series; (first, last) calendar years or datetime64 values, inclusive).

    The means are exact integer sums on the device: sum_q = the sum of rint((x - offset) * 2**16) over the valid steps
    of a month, mean = offset + sum_q / n_valid / 2**16.  Samples must lie within 2**7 of ``offset`` (kelvin: 273.15).
    Returns a MonthlyMeanDataset (mmm, monthly_mean, n_valid, sum_q); heat_stress() takes it as ``base``.  ``_compute``:
    a stand-in for class_sums_cells() (host tests)."""
    layout = grid_layout(temp, tdim)
    coords, _, dims, point, sdims, sshape, N = layout
    time = np.asarray(coords[tdim])
    kid = _period_labels(time, period)
    offset = float(offset)
    if not np.isfinite(offset):
        raise XmhwException(f"offset should be finite, got {offset!r}")
    # what rides in the place of the climatologies: one row that is NaN on land, so that the series' survivors pair
    # with the accumulators' columns
    land = zero_base(ocean_mask(temp, dims, tdim, point, anynans), point, sdims, sshape, coords)
    f, (nv, sq), _ = cell_stage(
        "class-sums", temp, land, land, layout, tdim,
        lambda host_keep, ts, sec, thc, doy, doys, options, **extra:
            (_compute or class_sums_cells)(ts, kid, 12, offset, **extra),
        lambda stacked, anynans_, sec, thc, doy, doys, options, **extra:
            class_sums_grid(stacked, anynans_, sec, kid, 12, offset, **extra),
        lambda C: [(12, C)] * 2, _SumsAccumulators.range_texts, anynans=anynans, _compute=_compute,
        max_batch_bytes=max_batch_bytes)
    return MonthlyMeanDataset(f.place(nv, 0, np.int32), f.place(sq, 0, np.int64), f.keep, f.sdims, f.coords, offset, period,
                              {"period": "all" if period is None else str(tuple(period))})


def degree_heating_weeks(temp, period=None, **kw):
    """Coral Reef Watch's Degree Heating Week: heat_stress() with its defaults (84 daily steps, 1 degree above the MMM,
    weeks, levels 4 and 8) against the maximum_monthly_mean() of ``temp`` over ``period``.  Keyword arguments go to
    heat_stress(); tdim, anynans and max_batch_bytes to both; ``offset`` to maximum_monthly_mean(); ``_compute``: a pair
    of stand-ins (class sums, stress)."""
    sums_compute, stress_compute = kw.pop("_compute", None) or (None, None)
    shared = {k: kw[k] for k in ("tdim", "anynans", "max_batch_bytes") if k in kw}
    mmm = maximum_monthly_mean(temp, period, offset=kw.pop("offset", 0.0), _compute=sums_compute, **shared)
    return heat_stress(temp, mmm, _compute=stress_compute, **kw)
