"""mhw_days_by(): per cell and per CLASS of time steps, how often the cell was in a heatwave, in which category, and how
hot it was -- seasonality maps of MHW days (classes = months or seasons), days counted in the year they fall in and the
highest category reached per year (Hobday et al. 2018, fig. 2), MHW occurrence by phase of a climate mode (Holbrook et
al. 2019: El Nino / La Nina / neutral days, see classes_from_events()).  mhw_coverage() and region_series() sum ACROSS
cells and keep the time axis; block_average(), mean_trend() and mhw_rank() reduce the event table and attribute a whole
event to the year it starts in.  This is the reduction over TIME that keeps the cell, and it cannot come from the table:
the per-step category and the anomaly are not constant along a row.  One streaming pass over the resident series, the
climatology and the in-event bitmap (csrc/kernels_class.hip).

The definition.  Inputs are those of mhw_coverage() plus ``class_of_t``: one int32 label per time step in [-1, K); -1
means the step counts nowhere.  A step t of cell c is *in an event* iff detect() labels it (mhw_filter() + join_gaps();
gap days of joined events included, exactly as in mhw_coverage()).  For each sample, with x = float64(ts[t, c]), negated
under coldSpells, and the climatology rows of t:
    a   = x - seas[row(t), c]                          (the expression of xmhw_event_stats_*)
    cat = floor(1 + (x - thresh) / (thresh - seas))    (the per-step category of mhw_df())
For every class k and cell c, over the in-event steps with class_of_t[t] == k:
    days[k, 0..3, c] (int32)   steps with cat == 1, == 2, == 3, >= 4 (moderate, strong, severe, extreme)
    days[k, 4, c]    (int32)   all in-event steps (event)
    days[k, 5, c]    (int32)   n_valid: in-event steps whose a is not NaN and |a| < 2**7 (the rule of mhw_track_intensity())
    isum_q[k, c]     (int64)   sum of rint(a * 2**16) over the valid steps        (INTENSITY_BITS = 16)
    intensity_max[k, c] (float64)  max a over the valid steps, NaN if there are none (-0.0 counts as 0.0): an integer
                     maximum of the order-preserving 64-bit key, exact and independent of the schedule.
An in-event step with a not NaN and |a| >= 2**7 is left out of n_valid, isum_q and intensity_max, is still counted in
days[k, 0..4, c], and is counted in n_range; mhw_days_by() raises if n_range > 0.  |isum_q| < 2**31 * 2**23: int64 cannot
overflow.  Everything is an integer sum or a maximum, so the result does not depend on the time blocks, the slabs, the
launch geometry or the schedule.

Host side here (validation, class labels, slabs, land); device side in csrc/kernels_class.hip behind class_days_cells()
(a compact host series) and class_days_grid() (a stacked grid, masked and compacted on the device slab by slab, as
coverage_grid()).
"""
import numpy as np

from .coverage import CATEGORIES
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .series_stage import (Accumulators, cell_stage, check_class_ids, class_labels, class_result_labels, dense_ids,
                           grid_layout, run_cells, run_grid, stage_attrs)     # (class_labels: imported from here too)

MAX_CLASSES = 1024              # XMHW_CLASS_DAYS_MAX_CLASSES (include/xmhw_amd.h)
CHANNELS = 6                    # XMHW_CLASS_DAYS_CHANNELS: CATEGORIES, then n_valid
INTENSITY_BITS = 16             # XMHW_TRACK_INTENSITY_BITS
RANGE_BITS = 7                  # |a| < 2**7
_RANGE_TEXT = ("in-event samples lie 2**7 and more from their climatology (or are infinite): is the series in kelvin "
               "and the climatology in degrees Celsius?")


def _check_classes(T, classes, K):
    return check_class_ids(T, classes, K, MAX_CLASSES, "mhw_days_by")


class _Accumulators(Accumulators):
    """One call's arguments and its device accumulators: days int32 (K, 6, C), isum_q int64 (K, C), intensity_max (K, C),
    which holds the order-preserving keys until finish() turns them into float64 in place, and the range counter."""
    range_texts = {"n_range": _RANGE_TEXT}

    def __init__(self, classes, K, minDuration, joinGaps, maxGap, coldSpells):
        super().__init__()
        self.classes, self.K = classes, K
        self.filter = (int(minDuration), int(bool(joinGaps)), int(maxGap))
        self.neg = int(bool(coldSpells))

    def begin(self, T, C):
        """T steps, C ocean cells"""
        self.classes, self.K = _check_classes(T, self.classes, self.K)
        K = self.K
        self.make(C, {"days": ((K, CHANNELS, C), np.int32), "isum_q": ((K, C), np.int64),
                      "intensity_max": ((K, C), np.float64)})
        with as_xmhw_errors(also="Unsupported"):
            self.h.class_days_init(K, C, *self.ptrs(), C, self.count.ptr)

    def add_slab(self, slab):
        """One slab (series_stage.Slab), columns k0..k0+n-1 of the accumulators: exceedance bits, then the reduction
        ADDS."""
        d_ts, T, n = slab.d_ts, slab.T, slab.n
        W = (T + 63) // 64
        with DeviceScope() as s:
            d_bits = s.alloc(8 * W * n)
            with as_xmhw_errors(also="Unsupported"):
                self.h.exceed_bits(d_ts.ptr, slab.isz, T, n, slab.ld, slab.th_ptr, slab.ldc, slab.D, slab.rows, self.neg,
                                   d_bits.ptr, n)
                self.h.class_days_accumulate(d_ts.ptr, slab.isz, T, n, slab.ld, slab.se_ptr, slab.th_ptr, slab.ldc, slab.rows,
                                             self.neg, d_bits.ptr, n, *self.filter, self.classes, self.K,
                                             *self.ptrs(slab.k0), self.C, self.count.ptr)
            self.h.stream_sync(0)                       # d_bits is freed on the way out

    def finish(self):
        with as_xmhw_errors(also="Unsupported"):
            self.h.class_days_finish(self.K, self.C, *self.ptrs(0, ("intensity_max",)), self.C)


def class_days_cells(ts, seas, thresh, doy, doys, classes, K, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False,
                     max_batch_bytes=64 << 30, pad=None, counters=None):
    """The device stage for a dense (T, C) series (arguments as detect_front.detect_cells): classes (T,) int labels in
    [-1, K).  Returns (days int32 (K, 6, C), isum_q int64 (K, C), intensity_max float64 (K, C)).  Cells go through the
    device in batches below max_batch_bytes, as in coverage_cells(); the sums are integers, so the batch size does not
    change a single bit.  Raises if a sample is out of range (module docstring); with ``counters`` (a dict) it stores
    ``n_range`` there instead."""
    return run_cells(_Accumulators(classes, K, minDuration, joinGaps, maxGap, coldSpells), ts, seas, thresh, doy, doys,
                     lambda T, isz, D: T * (isz + 1) + T // 4 + 2 * D * 8 + 64, max_batch_bytes, pad, counters)


def class_days_grid(stacked, anynans, seas, thresh, doy, doys, classes, K, minDuration=5, joinGaps=True, maxGap=2,
                    coldSpells=False, max_batch_bytes=None, clim_stacked=False, pad=None, counters=None):
    """class_days_cells() for an UNCOMPACTED stacked host series (T, N), float or a packed int16 view, as coverage_grid():
    the land mask and the compaction run on the device slab by slab (series_stage.walk_grid).  The accumulators live
    across the slabs and each slab writes its own column range.  Returns (days, isum_q, intensity_max, keep[N]) over the
    ocean cells."""
    out, keep = run_grid(_Accumulators(classes, K, minDuration, joinGaps, maxGap, coldSpells), stacked, anynans, seas,
                         thresh, doy, doys, lambda T, D: 6 * D * 8 + T // 4 + 64, max_batch_bytes, clim_stacked, pad, counters)
    return out + (keep,)


def classes_from_events(T, *event_datasets):
    """Class labels from the events of single-point series: class 0 everywhere, class i + 1 on the steps index_start ..
    index_end of the i-th EventDataset; a later dataset wins where two overlap.  With the warm and the cold-spell
    detect() of a Nino-3.4 ``region_series().series()`` this gives neutral / El Nino / La Nina days."""
    from .detect import EventDataset
    T = int(T)
    out = np.zeros(T, dtype=np.int32)
    for i, ev in enumerate(event_datasets):
        if not isinstance(ev, EventDataset):
            raise XmhwException("classes_from_events expects the EventDatasets returned by xmhw_amd.detect()")
        if not ev.point:
            raise XmhwException("classes_from_events expects events of single-point series (e.g. of region_series().series()), "
                                "got a gridded dataset")
        if np.asarray(ev.time).shape[0] != T:
            raise XmhwException(f"event dataset {i} has {np.asarray(ev.time).shape[0]} time steps, expected {T}")
        rows = ev.compact_view()
        for s, e in zip(rows["start"], rows["end"]):
            if e >= T:
                raise XmhwException("index_end outside the time axis")
            out[int(s):int(e) + 1] = i + 1
    return out


class ClassDaysDataset:
    """What mhw_days_by() returns, as plain arrays over (klass, [category,] *spatial dims).

    klass (K,) the class labels (sorted non-negative labels found), n_steps (K,) the time steps of each class;
    category = coverage.CATEGORIES (moderate, strong, severe, extreme, event);
    days int32 (K, 5, ...), n_valid int32 (K, ...), isum_q int64 (K, ...), intensity_max float64 (K, ...);
    frequency = days[event] / n_steps; intensity_mean = isum_q / (n_valid * 2**16), NaN where n_valid == 0;
    category_max int8 (K, ...), 0..4: the highest category with a non-zero day count (0: none).
    Land: grid lines without an ocean cell are dropped, as in BlockDataset; float fields are NaN on the remaining land
    cells, integer fields are 0 there and come with the boolean ``keep`` (...) mask of the ocean cells."""

    def __init__(self, klass, n_steps, days, n_valid, isum_q, intensity_max, keep, sdims, coords, tdim="time", attrs=None):
        self.klass, self.n_steps, self.category = np.asarray(klass), np.asarray(n_steps), CATEGORIES
        self.days, self.n_valid, self.isum_q, self.intensity_max = days, n_valid, isum_q, intensity_max
        self.keep, self.sdims, self.coords = keep, tuple(sdims), dict(coords)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        bshape = (-1,) + (1,) * (days.ndim - 2)
        land = ~np.broadcast_to(keep, n_valid.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.frequency = days[:, 4].astype(np.float64) / self.n_steps.astype(np.float64).reshape(bshape)
            self.intensity_mean = isum_q.astype(np.float64) / (n_valid.astype(np.float64) * float(1 << INTENSITY_BITS))
        self.intensity_mean[n_valid == 0] = np.nan
        self.frequency[land] = np.nan
        cmax = np.zeros(n_valid.shape, dtype=np.int8)
        for j in range(4):
            cmax[days[:, j] > 0] = j + 1
        self.category_max = cmax

    @staticmethod
    def quantisation_bound():
        """Bound on |intensity_mean - the float64 mean of a over the valid steps| from the fixed point alone: every
        rint(a * 2**16) / 2**16 is within 2**-17 of its a (the product by 2**16 is exact), so the exact ratio isum_q /
        (n_valid * 2**16) is within 2**-17 of the true mean.  In float64, n_valid * 2**16 is exact, isum_q (below 2**54
        in magnitude) converts with a relative error of 2**-53 at most, and the one division rounds by half an ulp: on
        a mean below 2**7 that is less than 2**-46 + 2**-47.  2**-17 + 2**-45 covers all of it."""
        return 2.0 ** -17 + 2.0 ** -45

    def to_xarray(self):
        import xarray as xr
        cell = ("klass",) + self.sdims
        return xr.Dataset(
            {"days": (("klass", "category") + self.sdims, self.days), "n_valid": (cell, self.n_valid),
             "isum_q": (cell, self.isum_q), "intensity_max": (cell, self.intensity_max),
             "frequency": (cell, self.frequency), "intensity_mean": (cell, self.intensity_mean),
             "category_max": (cell, self.category_max), "n_steps": (("klass",), self.n_steps),
             "keep": (self.sdims, self.keep)},
            coords=dict({"klass": self.klass, "category": list(CATEGORIES)}, **{d: self.coords[d] for d in self.sdims}),
            attrs=self.attrs)


def mhw_days_by(temp, th, se, classes="month", tdim="time", minDuration=5, joinGaps=True, maxGap=2, maxPadLength=None,
                coldSpells=False, tstep=False, anynans=False, _compute=None, max_batch_bytes=None):
    """Per cell and per class of time steps: MHW days by category, and the mean and maximum anomaly of those days.

    ``temp``, ``th``, ``se`` and the options shared with detect() mean and validate what they do there and in
    mhw_coverage() (same exceptions, land masking and positional pairing of series and climatology cells).
    ``classes``: an integer array with one label per time step, or "all", "month" (1..12), "season" (DJF, MAM, JJA, SON
    = 0..3) or "year", taken from a datetime64 time coordinate.  Negative labels count nowhere; the classes of the
    result are the sorted non-negative labels found (at most MAX_CLASSES).  classes_from_events() builds the labels of
    the phases of a climate mode from detect() on an index series.

    Returns a ClassDaysDataset.  Raises if an in-event sample lies 2**7 and more from its climatology.  ``_compute``: a
    stand-in for class_days_cells() (host tests)."""
    layout = grid_layout(temp, tdim)
    coords, _, _, point, sdims, sshape, N = layout
    time = np.asarray(coords[tdim])
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "mhw_days_by", "classes")
    n_steps = np.bincount(kid[kid >= 0], minlength=K).astype(np.int64)
    f, (days6, isum, imax), mhw = cell_stage(
        "class", temp, th, se, layout, tdim,
        lambda host_keep, ts, sec, thc, doy, doys, options, **extra:
            (_compute or class_days_cells)(ts, sec, thc, doy, doys, kid, K, *options, **extra),
        lambda stacked, anynans_, sec, thc, doy, doys, options, **extra:
            class_days_grid(stacked, anynans_, sec, thc, doy, doys, kid, K, *options, **extra),
        lambda C: [(K, CHANNELS, C), (K, C), (K, C)], _Accumulators.range_texts, based=False, maxPadLength=maxPadLength,
        coldSpells=coldSpells, tstep=tstep, anynans=anynans, _compute=_compute, max_batch_bytes=max_batch_bytes,
        detect_options=(minDuration, joinGaps, maxGap))
    attrs = stage_attrs(classes, mhw)
    return ClassDaysDataset(class_result_labels(found), n_steps, f.place(days6[:, :5], 0, np.int32),
                            f.place(days6[:, 5], 0, np.int32), f.place(isum, 0, np.int64), f.place(imax, np.nan, np.float64),
                            f.keep, f.sdims, f.coords, tdim, attrs)
