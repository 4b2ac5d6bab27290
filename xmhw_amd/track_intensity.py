"""mhw_track_intensity(): how hot every object of mhw_objects() was on each of its days -- the daily mean and maximum
anomaly over the object's footprint, its cumulative intensity, and how much of it was Moderate, Strong, Severe or
Extreme -- aligned with the ragged (CSR) arrays of mhw_tracks(): entry tr.offsets[i] + (t - tr.time_start[i]) belongs
to object tr.ids[i] on time position t.  The tracking tools of the field loop regionprops with an intensity image over
a dense labelled volume.  Every earlier object stage could avoid visiting voxels, because its quantities are constant
along a table row; this one cannot: it is the first reduction that joins the resident series, the climatology and the
object partition, one streaming pass over the series (csrc/kernels_track_intensity.hip).

The definition.  For a selected object o and a position t, take the voxels of o on t: the cells c that hold a row of o
with index_start <= t <= index_end (gap days of joined events included).  With x = float64(ts[t, c]), negated under
coldSpells, and the climatology rows of t:
    a[t, c] = x - seas[row(t), c]
the anomaly as the event statistics of detect() form it (xmhw_event_stats_*: the series is negated, the climatologies
are those of the negated series; the sign is the device's, positive for a cold spell too, before detect() flips the
table).  A voxel is *valid* iff a is not NaN.  Over the valid voxels:
    n_valid (int32) = their number,                 wsum_i (int64) = sum wi[c],
    isum_q (int64)  = sum wi[c] * aq[t, c],         aq = rint(a * 2**16)   (INTENSITY_BITS = 16),
    intensity_max (float64) = the largest a (NaN where there is none; -0.0 counts as 0.0, as in mhw_objects()): an
        integer maximum of the order-preserving 64-bit key, exact and independent of the schedule,
    cat_cells (4, L) int32 = the voxels whose per-step category floor(1 + (x - thresh) / (thresh - seas)), in float64,
        is 1, 2, 3 or >= 4: the semantics of mhw_coverage(); a voxel below the threshold or NaN is in none of the four.
A valid voxel with |a| >= 2**7, or infinite, is left out of every sum and counted, and the call raises: no value
outside the stated bound ever reaches a sum.

The bit budget.  wi = rint(w / w.max() * 2**ib) with ib = min(obj.weight_bits, 61 - 16 - 7 - bit_length(C)), C = the
ocean cells of the grid.  A day of an object holds at most C voxels, wi <= 2**ib and |aq| <= 2**23, so
|isum_q| <= C * 2**(ib + 23) < 2**(bit_length(C) + ib + 23) <= 2**61, whatever the data.  ib < 1 is refused.

Derived on the host, in float64: intensity_mean = isum_q / (wsum_i * 2**16) (NaN where wsum_i == 0); per object
intensity_cumulative = the sum of its defined intensity_mean, intensity_peak = the largest intensity_max of its days
and pos_peak, the first position that attains it (NaN and -1 for an object without a valid voxel).

Host side here (validation, selection, weights, slabs); device side in csrc/kernels_track_intensity.hip behind
track_intensity_cells() (a compact host series) and track_intensity_grid() (a stacked grid, masked and compacted on the
device slab by slab, as coverage_grid()).
"""
import numpy as np

from .detect import EventDataset
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .gridweights import quantise_weights, resolve_weights, weights_label
from .objects import ObjectDataset
from .series_stage import Accumulators, grid_layout, run, run_cells, run_grid
from .track_common import ChainDataset, Selection
from .tracks import TrackDataset

INTENSITY_BITS = 16             # XMHW_TRACK_INTENSITY_BITS (include/xmhw_amd.h)
RANGE_BITS = 7                  # |a| < 2**7
CATEGORIES = ("moderate", "strong", "severe", "extreme")
STAGE_FIELDS = ("n_valid", "wsum_i", "isum_q", "intensity_max", "cat_cells")
_STAGE = dict(n_valid=np.int32, wsum_i=np.int64, isum_q=np.int64, intensity_max=np.float64, cat_cells=(np.int32, 4))
_COLD_TEXT = "cold events were detected"


def intensity_bits(weight_bits, n_ocean):
    """ib of the module docstring"""
    return int(min(int(weight_bits), 61 - INTENSITY_BITS - RANGE_BITS - int(n_ocean).bit_length()))


def selection_rows(mhw, obj, tr):
    """The Selection (track_common.py) of ``tr``: the rows of ``mhw`` (start, end, slot; int32: the position of their object
    in ``tr.ids``, -1: not selected) with the (C + 1,) int64 row_offsets of the cells' rows, and the ragged layout of ``tr``
    (time_start (m,) int32, offsets (m + 1,) int64, m, L), checked against ``obj``."""
    return Selection.of_tracks(mhw, obj, tr, "mhw_track_intensity")


class _Accumulators(Accumulators):
    """One call's arguments and its device accumulators, one entry per day of every selected object (L in all): they are
    not sliced by column, every slab adds to them whole.  Two counters, out-of-range voxels and voxels outside their
    object's days, come back in the stage dict: the public function words their refusals."""

    def __init__(self, rows, wi, coldSpells):
        super().__init__()
        self.rows, self.wi, self.neg = rows, wi, int(bool(coldSpells))
        self.L, self.m = rows.L, rows.m

    def begin(self, T=None, C=None):
        """C: the cells of a dense series, which the table and the weights have to match"""
        rows, s = self.rows, self._scope
        if C is not None and (rows.row_offsets.shape != (C + 1,) or np.shape(self.wi) != (C,)):
            raise XmhwException("the table does not have one block of rows per ocean cell of temp: mhw does not belong to temp")
        L = self.L
        self.make(None, {"n_valid": ((L,), np.int32), "wsum_i": ((L,), np.int64), "isum_q": ((L,), np.int64),
                         "intensity_max": ((L,), np.float64), "cat_cells": ((4, L), np.int32)}, counters=2)
        self.time_start, self.offsets = s.upload(rows.time_start), s.upload(rows.offsets)
        with as_xmhw_errors(also="Unsupported", hint="select fewer objects with ids= in mhw_tracks()"):
            self.h.track_intensity_init(self.L, *self._out())

    def _out(self):
        return (*self.ptrs(), max(self.L, 1), self.count.ptr, self.count.ptr + 8)

    def add_slab(self, slab):
        """One slab (series_stage.Slab), the compact cells k0..k0 + n - 1: upload its rows, queue the pass"""
        rows, k0, n = self.rows, slab.k0, slab.n
        r0, r1 = int(rows.row_offsets[k0]), int(rows.row_offsets[k0 + n])
        if r1 == r0 or self.L == 0 or self.m == 0:
            return
        with DeviceScope() as s:
            d_start, d_end, d_slot = (s.upload(a[r0:r1]) for a in (rows.start, rows.end, rows.slot))
            d_roff = s.upload(rows.row_offsets[k0:k0 + n + 1] - r0)
            d_wi = s.upload(np.ascontiguousarray(self.wi[k0:k0 + n], dtype=np.int64))
            with as_xmhw_errors(also="Unsupported", hint="select fewer objects with ids= in mhw_tracks()"):
                self.h.track_intensity_accumulate(slab.d_ts.ptr, slab.isz, slab.T, n, slab.ld, slab.se_ptr, slab.th_ptr,
                                                  slab.ldc, slab.D, slab.rows, self.neg, d_start.ptr, d_end.ptr, d_slot.ptr,
                                                  r1 - r0, d_roff.ptr, d_wi.ptr, self.time_start.ptr, self.offsets.ptr,
                                                  self.m, self.L, *self._out())
            self.h.stream_sync(0)                       # the slab's rows are freed on the way out

    def finish(self):
        with as_xmhw_errors(also="Unsupported"):
            self.h.track_intensity_finish(self.L, *self.ptrs(0, ("intensity_max",)))

    def result(self):
        """(the stage dict: STAGE_FIELDS and the counters n_range and n_bad, no range to report)"""
        arrays, _ = super().result()
        n_range, n_bad = self.counts()
        return dict(zip(STAGE_FIELDS, arrays), n_range=n_range, n_bad=n_bad), {}


def track_intensity_cells(ts, seas, thresh, doy, doys, rows, wi, coldSpells=False, max_batch_bytes=64 << 30, pad=None):
    """The device stage for a dense (T, C) host series (arguments as coverage.coverage_cells): ``rows`` the selection_rows()
    of the selection, ``wi`` (C,) int64 weights.  Returns a dict of STAGE_FIELDS plus the counters n_range and n_bad.  Cells go
    through the device in batches below max_batch_bytes; the sums are integers, so the batch size does not change a bit."""
    return run_cells(_Accumulators(rows, wi, coldSpells), ts, seas, thresh, doy, doys, lambda T, isz, D: T * isz + 2 * D * 8 + 64,
                     max_batch_bytes, pad)


def track_intensity_grid(stacked, anynans, seas, thresh, doy, doys, rows, wi, keep_want, coldSpells=False,
                         max_batch_bytes=None, clim_stacked=False, pad=None):
    """track_intensity_cells() for an UNCOMPACTED stacked host series (T, N), as coverage.coverage_grid: the land mask and
    the compaction run on the device slab by slab (series_stage.walk_grid).  ``keep_want`` (N,) bool: the land mask of the
    detection; a slab whose mask differs is refused before it is used.  Returns (the stage dict, keep[N])."""
    N = stacked.shape[1]
    if keep_want.shape != (N,):
        raise XmhwException(f"temp has {N} grid points, the detection {keep_want.shape[0]}: mhw does not belong to temp")

    def check_keep(lo, hi, keep):
        if not np.array_equal(keep, keep_want[lo:hi]):
            raise XmhwException("the land mask of temp differs from mhw.keep: mhw does not belong to temp")

    return run_grid(_Accumulators(rows, wi, coldSpells), stacked, anynans, seas, thresh, doy, doys, lambda T, D: 6 * D * 8 + 64,
                    max_batch_bytes, clim_stacked, pad, begin_with=(), check_keep=check_keep)


class TrackIntensityDataset(ChainDataset):
    """What mhw_track_intensity() returns, as plain arrays, aligned with the TrackDataset it was given: m objects, L =
    offsets[-1] entries; entry offsets[i] + (t - time_start[i]) belongs to object ids[i] on time position t.

    ids, offsets, time_start, time_end, duration, pos    those of the TrackDataset, unchanged;
    n_valid (L,) int32              voxels of the object on that day with a defined anomaly;
    wsum_i, isum_q (L,) int64       the sums of wi and of wi * rint(a * 2**16) over them (module docstring);
    intensity_mean (L,) float64     isum_q / (wsum_i * 2**16): the weighted mean anomaly (NaN where wsum_i == 0);
    intensity_max (L,) float64      the largest anomaly of the day (NaN where n_valid == 0);
    cat_cells (4, L) int32          voxels in category moderate, strong, severe, extreme (CATEGORIES);
    intensity_cumulative (m,)       the sum of the object's defined intensity_mean (0 where none is);
    intensity_peak (m,), pos_peak (m,) int32    the largest intensity_max of the object's days and the first position
                                    that attains it (NaN, -1 for an object without a valid voxel);
    intensity_weight_bits (ib), n_ocean (C)."""

    _SERIES = ("pos", "n_valid", "wsum_i", "isum_q", "intensity_mean", "intensity_max")
    _PER_OBJECT = ("ids", "time_start", "time_end", "duration", "intensity_cumulative", "intensity_peak", "pos_peak")
    _ATTRS = ("intensity_bits", "intensity_weight_bits")
    _COORDS = {"category": list(CATEGORIES)}
    intensity_bits = INTENSITY_BITS

    def __init__(self, fields, time, sdims, sshape, intensity_weight_bits, n_ocean, attrs=None):
        super().__init__(fields, time, sdims, sshape, attrs)
        self.intensity_weight_bits, self.n_ocean = int(intensity_weight_bits), int(n_ocean)
        self.category = CATEGORIES

    def series(self, i):
        """The slices of the i-th selected object: a dict of its series (cat_cells as (4, days)) plus ``time``."""
        out = super().series(i)
        time = out.pop("time")                         # cat_cells comes in front of time, as it always did
        out.update(cat_cells=self.cat_cells[:, self._span(i)], time=time)
        return out

    def quantisation_bound(self):
        """(L,) float64: a bound on |intensity_mean - sum(w a) / sum(w)| over the valid voxels of every entry, for the
        unquantised float64 weights w and anomalies a.  Derived from the two roundings, not fitted.

        Write s = 2**ib / w.max().  The stored numbers are wi[c] = s w[c] + d[c], |d[c]| <= 1/2, and aq = 2**16 a + r,
        |r| <= 1/2.  First rounding: sum(wi aq) / (2**16 sum wi) = sum(wi a) / sum(wi) + sum(wi r) / (2**16 sum wi), and
        the second term is a weighted mean of r / 2**16: at most 2**-17.  Second rounding: with mu = sum(w a) / sum(w)
        (sum w > 0 whenever sum wi > 0: a zero weight is quantised to 0),
            sum(wi a) / sum(wi) - mu = sum(wi (a - mu)) / sum(wi) = sum(d (a - mu)) / sum(wi),
        because sum(s w (a - mu)) = 0.  mu lies among the a, all within (-2**7, 2**7), so |a - mu| < 2**8 and the term is
        below n_valid * 2**7 / wsum_i.  The float64 evaluation (two conversions and a division of a value below 2**7)
        adds less than 2**-44.  NaN where wsum_i == 0."""
        with np.errstate(divide="ignore", invalid="ignore"):
            b = self.n_valid.astype(np.float64) * 2.0 ** RANGE_BITS / self.wsum_i.astype(np.float64)
        return np.where(self.wsum_i > 0, b + 2.0 ** -(INTENSITY_BITS + 1) + 2.0 ** -44, np.nan)

    def _variables(self):
        return dict(super()._variables(), cat_cells=(("category", "obs"), self.cat_cells))


def mhw_track_intensity(temp, th, se, mhw, obj, tr, weights=None, tdim="time", maxPadLength=None, coldSpells=False,
                        tstep=False, anynans=False, _compute=None, max_batch_bytes=None):
    """The daily intensity and category series of the objects of mhw_tracks().

    ``temp``, ``th``, ``se`` and the options shared with detect() mean and validate what they do in mhw_coverage() (same
    exceptions, land masking, positional pairing of series and climatology cells, ``maxPadLength`` applied to the device
    copy of the series); give what detect() was given.  ``mhw``, ``obj``, ``tr``: the EventDataset of that detect(), the
    ObjectDataset of mhw_objects() and the TrackDataset of mhw_tracks() for it; the result uses ``tr.ids``,
    ``tr.offsets``, ``tr.time_start`` and ``tr.pos`` unchanged.  ``weights``: as for mhw_tracks(), and the same ones
    (they weight the mean).

    Returns a TrackIntensityDataset (module docstring: the definition; class docstring: the fields).  Every integer is
    a sum of integers and the maximum is an integer maximum: exact, and the same from run to run and for every
    ``max_batch_bytes``.  ``_compute``: a stand-in for track_intensity_cells() (host tests)."""
    if not isinstance(mhw, EventDataset):
        raise XmhwException("mhw_track_intensity expects the EventDataset returned by xmhw_amd.detect()")
    if not isinstance(obj, ObjectDataset):
        raise XmhwException("mhw_track_intensity expects the ObjectDataset returned by xmhw_amd.mhw_objects()")
    if not isinstance(tr, TrackDataset):
        raise XmhwException("mhw_track_intensity expects the TrackDataset returned by xmhw_amd.mhw_tracks()")
    if mhw.point:
        raise XmhwException("mhw_track_intensity needs a grid: a single-point series has no objects")
    if weights_label(weights) != tr.attrs.get("weights"):
        raise XmhwException(f"tr was made with weights {tr.attrs.get('weights')!r}, got {weights_label(weights)!r}: give "
                            "mhw_track_intensity() the weights mhw_tracks() was given")
    params = mhw.attrs.get("xmhw_parameters")
    if params is not None and (_COLD_TEXT in params) != bool(coldSpells):
        raise XmhwException(f"coldSpells={bool(coldSpells)} differs from the detection's recorded parameters")
    layout = grid_layout(temp, tdim)
    coords, _, _, point, sdims, sshape, _ = layout
    if point:
        raise XmhwException("mhw_track_intensity needs a grid: a single-point series has no objects")
    sshape = tuple(int(v) for v in sshape)
    if tuple(mhw.sdims) != tuple(sdims) or tuple(int(v) for v in mhw.sshape) != sshape:
        raise XmhwException(f"temp is on the grid {dict(zip(sdims, sshape))}, the detection on "
                            f"{dict(zip(mhw.sdims, mhw.sshape))}: mhw does not belong to temp")
    T = int(np.asarray(coords[tdim]).shape[0])
    if np.asarray(mhw.time).shape[0] != T:
        raise XmhwException(f"temp has {T} time steps, the detection {np.asarray(mhw.time).shape[0]}")
    rows = selection_rows(mhw, obj, tr)
    C = rows.C
    ib = intensity_bits(obj.weight_bits, C)
    if ib < 1:
        raise XmhwException(f"a grid of {sshape} with {C} ocean cells leaves no bits for the intensity weights")
    w = resolve_weights(weights, mhw.coords, list(sdims), None, list(sdims), sshape)
    wi = quantise_weights(w, ib)[0][rows.cell_index]
    keep_want = np.asarray(mhw.keep, dtype=bool).reshape(-1)
    got = {}

    def on_cells(host_keep, ts, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, **extra):
        # _detect() has masked and compacted on the host (a stand-in device stage)
        if not np.array_equal(host_keep(), keep_want):
            raise XmhwException("the land mask of temp differs from mhw.keep: mhw does not belong to temp")
        got["stage"] = (_compute or track_intensity_cells)(ts, sec, thc, doy, doys, rows, wi, coldSpells, **extra)

    def on_grid(stacked, anynans_, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, **extra):
        got["stage"], keep = track_intensity_grid(stacked, anynans_, sec, thc, doy, doys, rows, wi, keep_want, coldSpells,
                                                  **extra)
        return keep

    run(temp, th, se, layout, tdim, on_cells, on_grid, maxPadLength, coldSpells, tstep, anynans, _compute, max_batch_bytes)
    st = got["stage"]
    if st.get("n_bad"):
        raise XmhwException(f"{st['n_bad']} voxels of table rows do not lie within their object's days: obj or tr does "
                            "not belong to mhw")
    if st.get("n_range"):
        raise XmhwException(f"{st['n_range']} voxels hold an anomaly of 2**{RANGE_BITS} and more in magnitude: are temp, th "
                            "and se in the same units, and se the climatology of temp?")
    f = dict(ids=tr.ids, offsets=tr.offsets, time_start=tr.time_start, time_end=tr.time_end, duration=tr.duration, pos=tr.pos)
    f.update(rows.stage_arrays(st, _STAGE, "track intensity"))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = f["isum_q"].astype(np.float64) / (f["wsum_i"].astype(np.float64) * 2.0 ** INTENSITY_BITS)
    f["intensity_mean"] = np.where(f["wsum_i"] > 0, mean, np.nan)
    if rows.m:
        f["intensity_cumulative"] = np.add.reduceat(np.where(np.isnan(f["intensity_mean"]), 0.0, f["intensity_mean"]),
                                                    rows.offsets[:-1])
    else:
        f["intensity_cumulative"] = np.zeros(0)
    peak, pos = rows.first_max(np.where(np.isnan(f["intensity_max"]), -np.inf, f["intensity_max"]))
    has = np.isfinite(peak)
    f["intensity_peak"], f["pos_peak"] = np.where(has, peak, np.nan), np.where(has, pos, -1).astype(np.int32)
    attrs = {"weights": weights_label(weights)}
    if params is not None:
        attrs["xmhw_parameters"] = params
    return TrackIntensityDataset(f, mhw.time, mhw.sdims, sshape, ib, C, attrs)
