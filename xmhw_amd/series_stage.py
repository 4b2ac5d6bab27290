"""The stage layer: what the stages that walk the series slab by slab share ("What 3.7, 3.11 and 3.16
share").  mhw_coverage(), mhw_track_intensity(), mhw_days_by(), heat_stress() / maximum_monthly_mean(),
index_regression(), mhw_composite() and lag_correlation() are each a ``begin(T, C)`` / ``add_slab(slab)`` pair on top of
the things that exist once, here:

* Slab                      one slab of cells on the device, as the slab methods take it;
* climatologies_on_device() seas / thresh whole on the device, compacted there if needed (detect_grid() uses it too);
* walk_cells(), walk_grid() the dense and the grid slab walker;
* Accumulators              the base of every stage's accumulator class: scope, named device arrays with the cell axis
                            last, their pointers at a column, the range counters, the read-back, free();
* run_cells(), run_grid(), report_range()   one stage call: an Accumulators object over a walker, freed whatever happens,
                            and what becomes of its out-of-range counts;
* run()                     the one shim around detect._detect();
* cell_stage(), class_result_labels(), stage_attrs()    the tail of the public per-cell functions: run(), the range
                            raise, the CellFrame and the shape check of what the stage returned;
* class_labels(), dense_ids(), check_class_ids(), check_weighted_cells(), check_steps(), check_view()    labels and the
                            stage-side checks of per-call and per-cell arguments;
* base_series(), constant_rows(), ocean_mask(), zero_base()    a base in the place of the climatologies;
* same_axis(), check_same_frame()   a second input on the grid and time axis of the first;
* regions_of_result()       the regions found on ocean cells (mhw_coverage(), region_series());
* CellFrame, grid_frame(), cells_to_grid()      per-cell results back on the grid;
* grid_layout()             the spatial layout of a GridSeries / DataArray.
"""
from collections import namedtuple

import numpy as np

from . import calendar as cal
from ._lib import hip
from .api import GridSeries, _from_xarray, _is_xarray
from .device import DeviceScope
from .exception import XmhwException

LAND_TEXT = "All points of grid are either land or NaN"
NAMED_CLASSES = ("all", "month", "season", "year")
MAX_STEPS = 1 << 17             # XMHW_*_MAX_STEPS (include/xmhw_amd.h) of the entries that pack a step into 17 bits


class Slab(namedtuple("Slab", "d_ts isz T n ld se_ptr th_ptr ldc D rows k0 cols")):
    """n cells whose (T, n) series is on the device (buffer d_ts, item size isz, leading dimension ld), with the
    climatologies at their column offset (device pointers se_ptr / th_ptr, leading dimension ldc, D rows; ``rows``: the
    climatology row of every time step).  k0: the position of the slab's first cell among the ocean cells.  cols: what
    selects the slab's cells from a per-cell host array -- a slice of the compact cells on the dense route, (lo, hi,
    keep) of the whole grid on the grid route."""
    __slots__ = ()

    def take(self, a):
        """the slab's entries of a per-cell host array (one entry per compact cell, or per grid point: see cols)"""
        if isinstance(self.cols, slice):
            return a[self.cols]
        lo, hi, keep = self.cols
        return a[lo:hi][keep]


def climatologies_on_device(scope, seas, thresh, anynans, clim_stacked):
    """(d_se, d_th, C): the climatologies whole on the device, owned by ``scope`` -- they are small next to the series --
    as they are, (D, C), or masked and compacted there (clim_stacked: (D, N') arrays on a grid)."""
    from .device import compact_columns
    if clim_stacked:
        d_th, keep_th = compact_columns(thresh, 0, thresh.shape[1], anynans)
        scope.adopt(d_th)
        d_se, keep_se = compact_columns(seas, 0, seas.shape[1], anynans)
        scope.adopt(d_se)
        C, Cse = int(keep_th.sum()), int(keep_se.sum())
        if C == 0 or Cse == 0:
            raise XmhwException(LAND_TEXT)
    else:
        d_th, d_se = scope.upload(thresh), scope.upload(seas)
        C, Cse = thresh.shape[1], seas.shape[1]
    if C != Cse:
        raise XmhwException(f"th and se do not have the same ocean cells: {C}, {Cse}")
    return d_se, d_th, C


def walk_cells(ts, seas, thresh, doy, doys, per_cell, max_batch_bytes, pad, on_slab, begin=None):
    """The dense walker: a host (T, C) series and its (D, C) climatologies go through the device in batches of cells
    below max_batch_bytes, ``per_cell(T, isz, D)`` bytes a cell; ``on_slab(slab)`` queues the stage's work on each and
    synchronises before it frees what it uploaded.  ``begin(T, C)`` runs once the inputs are checked, before the first
    batch: the stage checks its own arguments against them and makes its accumulators there."""
    from .detect_front import _check_inputs
    ts, seas, thresh, rows = _check_inputs(ts, seas, thresh, doy, doys)
    T, C = ts.shape
    D = thresh.shape[0]
    isz = ts.dtype.itemsize
    if begin is not None:
        begin(T, C)
    batch = int(max(1, min(C, max_batch_bytes // max(per_cell(T, isz, D), 1))))
    for c0 in range(0, C, batch):
        c1 = min(C, c0 + batch)
        n = c1 - c0
        with DeviceScope() as s:
            d_ts = s.upload(np.ascontiguousarray(ts[:, c0:c1]))
            if pad is not None:
                pad.apply(d_ts.ptr, isz, T, n)
            d_se = s.upload(np.ascontiguousarray(seas[:, c0:c1]))
            d_th = s.upload(np.ascontiguousarray(thresh[:, c0:c1]))
            on_slab(Slab(d_ts, isz, T, n, n, d_se.ptr, d_th.ptr, n, D, rows, c0, slice(c0, c1)))


def walk_grid(stacked, anynans, seas, thresh, doy, doys, per_cell_extra, max_batch_bytes, clim_stacked, pad, on_slab,
              check_keep=None, begin=None):
    """The grid walker, for an UNCOMPACTED stacked host series (T, N), float or a packed int16 view, as
    detect_front.detect_grid: the land mask and the compaction run on the device slab by slab, the climatologies are
    compacted there as well (clim_stacked) and pair up with the series' survivors by POSITION.  ``per_cell_extra(T, D)``:
    the stage's bytes per cell on top of device._grid_batch()'s own.  ``on_slab(slab)`` as in walk_cells();
    ``begin(T, C)`` runs once the climatologies are on the device (C: their ocean cells); ``check_keep(lo, hi, keep)``
    sees the land mask of every slab, an all-land one included, before the slab is used.  Returns keep[N]."""
    from .detect_front import _check_inputs, _rows_as_they_are
    from .device import _grid_batch, compact_columns, device_itemsize, is_packed, native_float
    T, N = stacked.shape
    if not is_packed(stacked):
        stacked = np.ascontiguousarray(native_float(stacked))
    seas, thresh = _rows_as_they_are(seas), _rows_as_they_are(thresh)
    if seas.ndim != 2 or thresh.ndim != 2 or seas.shape[0] != thresh.shape[0]:
        raise XmhwException("seas and thresh must be (D, cells) arrays")
    D = thresh.shape[0]
    sample_dtype = stacked.decoded_dtype if is_packed(stacked) else stacked.dtype
    _, _, _, rows = _check_inputs(np.zeros((T, 1), dtype=sample_dtype), seas[:, :1], thresh[:, :1], doy, doys)
    isz = device_itemsize(stacked)
    keeps = []
    k0 = 0
    with DeviceScope() as clim:
        d_se, d_th, C = climatologies_on_device(clim, seas, thresh, anynans, clim_stacked)
        if begin is not None:
            begin(T, C)
        cb = _grid_batch(stacked, max_batch_bytes, per_cell_extra=per_cell_extra(T, D))
        for lo in range(0, N, cb):
            hi = min(N, lo + cb)
            d_ts, keep = compact_columns(stacked, lo, hi, anynans)
            keeps.append(keep)
            n = int(keep.sum())
            with DeviceScope() as s:
                s.adopt(d_ts)
                if check_keep is not None:
                    check_keep(lo, hi, keep)
                if d_ts is None:                        # an all-land slab: k0 stays
                    continue
                if pad is not None:
                    pad.apply(d_ts.ptr, isz, T, n)
                if k0 + n > C:
                    raise XmhwException(f"temp has more ocean cells than th and se ({C})")
                on_slab(Slab(d_ts, isz, T, n, n, d_se.ptr + 8 * k0, d_th.ptr + 8 * k0, C, D, rows, k0, (lo, hi, keep)))
            k0 += n
        keep = np.concatenate(keeps) if keeps else np.zeros(0, dtype=bool)
        if not keep.any():
            raise XmhwException(LAND_TEXT)
        if k0 != C:
            raise XmhwException(f"temp has {k0} ocean cells, th and se have {C}")
    return keep


def grid_layout(temp, tdim):
    """(coords, coord_attrs, dims, point, sdims, sshape, N) of a GridSeries / DataArray: the spatial dims in stacked
    (sorted-name) order, their shape and the number of grid points (1 for a single-point series)."""
    if _is_xarray(temp):
        coords, coord_attrs = _from_xarray(temp)
        dims = list(temp.dims)
    else:
        coords, coord_attrs, dims = dict(temp.coords), None, list(temp.dims)
    if tdim not in dims:
        raise XmhwException(f"{tdim} dimension not present, default"
                            + "is 'time' or pass as tdim='time_dimension_name'")
    point = len(dims) == 1
    sdims = sorted(d for d in dims if d != tdim)
    shape = tuple(temp.shape) if _is_xarray(temp) else tuple(np.shape(temp.values))
    sshape = tuple(shape[dims.index(d)] for d in sdims)
    N = int(np.prod(sshape, dtype=np.int64)) if not point else 1
    return coords, coord_attrs, dims, point, sdims, sshape, N


def run(temp, th, se, layout, tdim, cells_stage, grid_stage, maxPadLength, coldSpells, tstep, anynans, _compute,
        max_batch_bytes, minDuration=5, joinGaps=True, maxGap=2):
    """detect._detect() around a stage that returns no event table: detect()'s validation, land masking, pairing of
    series and climatology cells and padding, with the stage in the place of the detection.  ``layout``: the
    grid_layout() of ``temp``.

    ``cells_stage(host_keep, ts, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, **extra)`` gets the
    series _detect() masked and compacted on the host (a single point, or a stand-in ``_compute``); ``extra`` holds
    ``pad`` when there is one and ``max_batch_bytes`` when it was given and the stage is the device's.  ``host_keep()``
    computes the (N,) land mask of ``temp`` on the host, for a stage that selects per-cell arguments by it.
    ``grid_stage(stacked, anynans, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, max_batch_bytes=,
    clim_stacked=, pad=)`` gets the uncompacted grid and returns keep[N]; it is not used with a stand-in.
    Returns the EventDataset of _detect(), without events: its keep, cell_index and attrs are the call's."""
    from .detect import _detect
    coords, coord_attrs, dims, point = layout[:4]

    def host_keep():
        return ocean_mask(temp, dims, tdim, point, anynans)

    def no_events(C, **more):
        return dict(table=np.zeros((0, 31)), offsets=np.zeros(C + 1, dtype=np.int64), inter=None, **more)

    def on_cells(ts, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, intermediate, pad=None):
        extra = {} if pad is None else {"pad": pad}
        if max_batch_bytes is not None and _compute is None:
            extra["max_batch_bytes"] = max_batch_bytes
        cells_stage(host_keep, ts, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, **extra)
        return no_events(ts.shape[1])

    def on_grid(stacked, anynans_, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, intermediate,
                clim_stacked=False, pad=None):
        keep = grid_stage(stacked, anynans_, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells,
                          max_batch_bytes=max_batch_bytes, clim_stacked=clim_stacked, pad=pad)
        return no_events(int(keep.sum()), keep=keep)

    series = GridSeries(temp.values, dims, coords, coord_attrs=coord_attrs) if _is_xarray(temp) else temp
    as_series = lambda a: GridSeries(a.values, a.dims, _from_xarray(a)[0]) if _is_xarray(a) else a   # noqa: E731
    return _detect(series, as_series(th), as_series(se), on_cells, tdim, minDuration, joinGaps, maxGap, maxPadLength,
                   coldSpells, False, anynans, tstep, grid_compute=None if _compute is not None else on_grid)


def class_labels(classes, time):
    """The ``classes`` argument as labels per time step: an integer array of length T as it is, or a named form taken from
    a datetime64 time axis -- "all" (one class 0), "month" (1..12), "season" (DJF, MAM, JJA, SON = 0..3), "year" (the
    calendar year)."""
    time = np.asarray(time)
    T = time.shape[0]
    if isinstance(classes, str):
        if classes not in NAMED_CLASSES:
            raise XmhwException(f"classes should be an integer array or one of {NAMED_CLASSES}, got {classes!r}")
        if classes == "all":
            return np.zeros(T, dtype=np.int64)
        if time.dtype.kind != "M":
            raise XmhwException(f"classes={classes!r} needs a datetime64 time coordinate, got {time.dtype}: pass the class "
                                "of every time step as an integer array instead")
        year, month, _, _ = cal._fields(time)
        if classes == "month":
            return month.astype(np.int64)
        if classes == "season":
            return (month % 12) // 3
        return year.astype(np.int64)
    labels = np.asarray(classes)
    if labels.dtype.kind not in "iu":
        raise XmhwException(f"classes should be an integer array, got {labels.dtype}")
    if labels.shape != (T,):
        raise XmhwException(f"classes should have one entry per time step ({T}), got shape {labels.shape}")
    return labels.astype(np.int64)


def dense_ids(labels, cap, who, what):
    """Integer labels as dense ids: (found, ids, K) with ``found`` the sorted non-negative labels, ``ids`` int32 the
    position of every label in it (-1: a negative label, which counts nowhere) and K = max(len(found), 1), at most
    ``cap``.  ``who`` and ``what`` (the caller, "regions" or "classes") word the message of the cap."""
    found = np.unique(labels[labels >= 0])
    ids = np.where(labels >= 0, np.searchsorted(found, labels), -1).astype(np.int32)
    K = max(int(found.shape[0]), 1)
    if K > cap:
        raise XmhwException(f"{who} handles at most {cap} {what}, got {K}")
    return found, ids, K


def check_class_ids(T, classes, K, cap, who):
    """The stage-side check of class ids: (classes int32 (T,) in [-1, K), K in [1, cap])"""
    classes = np.asarray(classes)
    if classes.dtype.kind not in "iu":
        raise XmhwException(f"classes should be an integer array, got {classes.dtype}")
    if classes.shape != (T,):
        raise XmhwException(f"classes should have one entry per time step ({T}), got shape {classes.shape}")
    K = int(K)
    if K < 1:
        raise XmhwException("K should be >= 1")
    if K > cap:
        raise XmhwException(f"{who} handles at most {cap} classes, got {K}")
    if T and (classes.min() < -1 or classes.max() >= K):
        raise XmhwException("class labels should be in [-1, K)")
    return np.ascontiguousarray(classes, dtype=np.int32), K


def check_weighted_cells(C, w, region, R, cap, who, name):
    """The stage-side check of per-cell integer weights in [0, 2**31] (``name`` in the message) and region ids in
    [-1, R), R in [1, cap]: (w int64 (C,), region int32 (C,), R)"""
    w = np.ascontiguousarray(w, dtype=np.int64)
    region = np.ascontiguousarray(region, dtype=np.int32)
    if w.shape != (C,) or region.shape != (C,):
        raise XmhwException(f"{name} and region should have one entry per cell")
    if C and (w.min() < 0 or w.max() > 1 << 31):
        raise XmhwException("quantised weights should be in [0, 2**31]")
    R = int(R)
    if R < 1:
        raise XmhwException("R should be >= 1")
    if C and (region.min() < -1 or region.max() >= R):
        raise XmhwException("region ids should be in [-1, R)")
    if R > cap:
        raise XmhwException(f"{who} handles at most {cap} regions, got {R}")
    return w, region, R


def regions_of_result(keep, rid, w, found):
    """The regions of a result are the labels found on OCEAN cells: (sel, ncells, total, region) with ``sel`` the mask
    over the candidate ids that selects them (None when every cell is excluded: one empty region 0), and their number of
    ocean cells, integer weight and label.  keep, rid, w: (N,) land mask, dense region ids and integer weights."""
    Rc = max(int(found.shape[0]), 1)
    ocean = keep & (rid >= 0)
    ncells = np.bincount(rid[ocean], minlength=Rc).astype(np.int64)
    total = np.zeros(Rc, dtype=np.int64)
    np.add.at(total, rid[ocean], w[ocean])
    if not found.shape[0]:
        return None, ncells, total, np.zeros(1, dtype=np.int64)
    sel = ncells > 0
    return sel, ncells[sel], total[sel], found[sel]


class Accumulators:
    """The base of a stage's accumulator class: the device arrays of one call, which live across the slabs -- each slab
    adds into its own column range -- and are read back once.  A stage adds ``begin(T, C)`` (its argument checks,
    make(), its init entry), ``add_slab(slab)`` (its launches) and, where it has one, ``finish()``; ``range_texts`` maps
    the key of each of its out-of-range counters to the text of the refusal, in the order of the counters."""
    range_texts = {}

    def __init__(self, scope=None):
        self.h, self.C = hip(), None
        self._scope = DeviceScope() if scope is None else scope
        self._table, self._buf, self.count = {}, {}, None

    def make(self, C, table, counters=None):
        """allocate the arrays of ``table``, name -> (shape, dtype) in the order they are read back, and ``counters``
        int64 range counters (default: one per range text).  C: the cells, the last axis of every shape (None: the
        arrays are not per cell)."""
        self.C, self._table = C, dict(table)
        self._buf = {k: self._scope.alloc(max(int(np.prod(shape)), 1) * np.dtype(dt).itemsize)
                     for k, (shape, dt) in self._table.items()}
        self.n_counters = len(self.range_texts) if counters is None else counters
        if self.n_counters:
            self.count = self._scope.alloc(8 * self.n_counters)

    def ptrs(self, k0=0, names=None):
        """the device pointers of the arrays (``names``: of those, in that order) at column k0"""
        return [self._buf[k].ptr + np.dtype(self._table[k][1]).itemsize * k0 for k in (names or self._table)]

    def read(self, names=None):
        """the arrays on the host, in table order; an empty one (no cells) is not read"""
        return tuple(self._buf[k].to_array(shape, dt) if int(np.prod(shape)) else np.zeros(shape, dt)
                     for k, (shape, dt) in ((k, self._table[k]) for k in (names or self._table)))

    def counts(self):
        """the range counters as ints"""
        if self.C == 0 or not self.n_counters:
            return (0,) * self.n_counters
        return tuple(int(v) for v in self.count.to_array((self.n_counters,), np.int64))

    def finish(self):
        """what a stage queues once after the last slab"""

    def result(self):
        """(the arrays, {key of range_texts: count})"""
        if self.C != 0:
            self.finish()
        self.h.stream_sync(0)
        return self.read(), dict(zip(self.range_texts, self.counts()))

    def free(self):
        self._scope.free()


def report_range(n_range, counters, texts):
    """What a stage does with its counts of samples outside the fixed-point range, ``n_range`` {key: count}: into
    ``counters`` (a dict) when the caller collects them, otherwise an exception worded by ``texts`` {key: text} for the
    first that is not zero."""
    if counters is not None:
        counters.update((k, int(v)) for k, v in n_range.items())
        return
    for k, v in n_range.items():
        if v:
            raise XmhwException(f"{int(v)} {texts[k]}")


def _run_stage(acc, walk, counters):
    try:
        keep = walk()
        out, n_range = acc.result()
    finally:
        acc.free()
    report_range(n_range, counters, acc.range_texts)
    return out, keep


def run_cells(acc, ts, seas, thresh, doy, doys, per_cell, max_batch_bytes, pad, counters=None):
    """One stage call over a dense series: the slabs of walk_cells() go through ``acc`` (an Accumulators), which is
    freed whatever happens; then the range counts are reported (report_range()).  Returns what acc.result() read."""
    return _run_stage(acc, lambda: walk_cells(ts, seas, thresh, doy, doys, per_cell, max_batch_bytes, pad, acc.add_slab,
                                              acc.begin), counters)[0]


def run_grid(acc, stacked, anynans, seas, thresh, doy, doys, per_cell_extra, max_batch_bytes, clim_stacked, pad,
             counters=None, begin_with=None, check_keep=None):
    """run_cells() over an uncompacted grid (walk_grid()).  ``begin_with``: None lets the walker call acc.begin(T, C)
    with the ocean cells of the climatologies; a tuple is what acc.begin() is called with before the walk, for a stage
    whose per-cell arguments are not those of the ocean cells.  ``check_keep``: as in walk_grid().  Returns (what
    acc.result() read, keep[N])."""
    def walk():
        if begin_with is not None:
            acc.begin(*begin_with)
        return walk_grid(stacked, anynans, seas, thresh, doy, doys, per_cell_extra, max_batch_bytes, clim_stacked, pad,
                         acc.add_slab, check_keep=check_keep, begin=acc.begin if begin_with is None else None)
    return _run_stage(acc, walk, counters)


def cell_stage(who, temp, th, se, layout, tdim, cells_stage, grid_stage, want, range_texts, based=True, maxPadLength=None,
               coldSpells=False, tstep=False, anynans=False, _compute=None, max_batch_bytes=None, detect_options=()):
    """The tail that the public per-cell functions share: run() around the two stages of one function, the refusal of
    out-of-range samples, the CellFrame of the result and the shape check of what the stage returned.

    ``cells_stage(host_keep, ts, sec, thc, doy, doys, options, **extra)`` returns the stage's arrays for the series that
    _detect() compacted on the host; ``grid_stage(stacked, anynans, sec, thc, doy, doys, options, **extra)`` returns them
    and keep[N].  ``options`` is (minDuration, joinGaps, maxGap, coldSpells); ``extra`` holds ``counters`` and what run()
    adds.  ``based``: th / se are a base, whose single row pairs with every step (constant_rows()).  ``want(C)``: the
    shapes expected for C cells; ``who`` names the stage in the message.  ``range_texts``: as Accumulators.range_texts.
    Returns (the CellFrame, the arrays, the EventDataset of run())."""
    got, counters = [], {}

    def on_cells(host_keep, ts, sec, thc, doy, doys, *options, **extra):
        if based:
            doy, doys = constant_rows(sec, doy, doys)
        got.extend(cells_stage(host_keep, ts, sec, thc, doy, doys, options, counters=counters, **extra))

    def on_grid(stacked, anynans_, sec, thc, doy, doys, *options, **extra):
        if based:
            doy, doys = constant_rows(sec, doy, doys)
        *out, keep = grid_stage(stacked, anynans_, sec, thc, doy, doys, options, counters=counters, **extra)
        got.extend(out)
        return keep

    mhw = run(temp, th, se, layout, tdim, on_cells, on_grid, maxPadLength, coldSpells, tstep, anynans, _compute,
              max_batch_bytes, *detect_options)
    for key, text in range_texts.items():
        if counters.get(key, 0):
            raise XmhwException(f"{counters[key]} {text}")
    coords, point, sdims, sshape = layout[0], layout[3], layout[4], layout[5]
    f = CellFrame(mhw.keep, mhw.cell_index, point, sdims, sshape, coords)
    arrays = [np.asarray(a) for a in got]
    if [a.shape for a in arrays] != list(want(f.C)):
        raise XmhwException(f"{who} stage returned {[a.shape for a in arrays]}, expected {want(f.C)}")
    return f, arrays, mhw


def class_result_labels(found):
    """the klass axis of a result: the labels found, or the one class 0 of a call that labels no step"""
    return found if found.shape[0] else np.zeros(1, dtype=np.int64)


def stage_attrs(classes, mhw, **more):
    """the attrs that the per-class results share, ``more`` between them"""
    return {"classes": classes if isinstance(classes, str) else "array", **more,
            "xmhw_parameters": mhw.attrs["xmhw_parameters"]}


# ---- a base in the place of the climatologies, a second input beside the first ------------------------------------

def constant_rows(sec, doy, doys):
    """a one-row baseline pairs with every step: its labels are not day-of-year labels"""
    if sec.shape[0] == 1:
        return np.zeros(np.asarray(doy).shape[0], dtype=np.int64), np.zeros(1, dtype=np.int64)
    return doy, doys


def base_series(base, point, sdims, coords):
    """``base`` as the GridSeries with a 'doy' dimension that pairs with the series like th / se; a result that stands
    for a base (MonthlyMeanDataset) says so with as_series()"""
    if hasattr(base, "as_series"):
        base = base.as_series()
    elif _is_xarray(base):
        base = GridSeries(base.values, base.dims, _from_xarray(base)[0])
    elif not isinstance(base, GridSeries):
        a = np.asarray(base, dtype=np.float64)
        nd = 0 if point else len(sdims)
        if a.ndim not in (nd, nd + 1):
            raise XmhwException(f"base should be a {tuple(sdims)} array or a ('doy',) + {tuple(sdims)} climatology, got "
                                f"shape {a.shape}")
        dims = tuple(sdims) if a.ndim == nd else ("doy",) + tuple(sdims)
        c = {d: coords[d] for d in sdims if d in coords}
        if "doy" in dims:
            c["doy"] = np.arange(1, a.shape[0] + 1)
        base = GridSeries(a, dims, c)
    if "doy" not in base.dims:
        base = GridSeries(np.asarray(base.values, dtype=np.float64)[None], ("doy",) + tuple(base.dims),
                          dict(base.coords, doy=np.zeros(1, dtype=np.int64)))
    return base


def ocean_mask(field, dims, tdim, point, anynans):
    """(N,) bool: the ocean cells of a field, computed on the host as _detect() masks them"""
    from .landmask import keep_mask, stack_cells
    if point:
        return np.array([True])
    values = field.values if hasattr(field, "values") else field
    return keep_mask(stack_cells(np.asarray(values), dims, tdim)[0], anynans)


def zero_base(ocean, point, sdims, sshape, coords):
    """A base of zero that pairs with the ocean cells of a field as a climatology does: one row, NaN on land."""
    values = 0.0 if point else np.where(ocean, 0.0, np.nan).reshape(sshape)
    return base_series(values, point, sdims, coords)


def same_axis(ta, tb):
    ta, tb = np.asarray(ta), np.asarray(tb)
    if ta.shape != tb.shape:
        return False
    try:
        return bool(np.array_equal(ta, tb))
    except (TypeError, ValueError):
        return False


def check_same_frame(who, first, second, layout, time, other_layout, other_time):
    """A second input (named ``second``) has to be on the grid and the time axis of the first: the layouts are (point,
    sdims, sshape)."""
    (point, sdims, sshape), (opoint, osdims, osshape) = layout, other_layout
    T, To = np.asarray(time).shape[0], np.asarray(other_time).shape[0]
    if bool(opoint) != bool(point):
        raise XmhwException(f"{who} cannot pair a single-point series with a grid")
    if not point and (tuple(osdims) != tuple(sdims) or tuple(osshape) != tuple(sshape)):
        raise XmhwException(f"{first} and {second} are not on the same grid: {tuple(sdims)} {tuple(sshape)} and "
                            f"{tuple(osdims)} {tuple(osshape)}")
    if To != T:
        raise XmhwException(f"{first} and {second} have {T} and {To} time steps")
    if not same_axis(time, other_time):
        raise XmhwException(f"{first} and {second} do not have the same time axis")


def check_steps(T, who):
    """the entries that pack a time step into 17 bits refuse a longer series"""
    if T >= MAX_STEPS:
        raise XmhwException(f"{who} handles fewer than 2**17 time steps, got {T}")


def check_view(view, cells, T, what):
    """What the rasteriser relies on, for the cells it will read: positions inside the table, 0 <= start <= end < T
    (compact_view() gives the first two) and the rows of a cell in time order."""
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    if cells.ndim != 1 or (cells.size and (cells.min() < 0 or cells.max() >= view["C"])):
        raise XmhwException(f"{what}: cell positions outside the table")
    start, end, offsets = view["start"], view["end"], view["offsets"]
    if view["n"]:
        if int(end.max()) >= T:
            raise XmhwException(f"{what}: index_end outside the time axis")
        later = np.diff(start.astype(np.int64)) < 0
        if later.any():
            first = np.zeros(view["n"], dtype=bool)              # rows that open a cell: no order across cells
            first[offsets[:-1][offsets[:-1] < view["n"]]] = True
            if (later & ~first[1:]).any():
                raise XmhwException(f"{what}: the rows of a cell are not in time order")
    return cells


class CellFrame:
    """Per-cell results on the grid of a call: a single point, or the grid with its dead lines dropped (grid_frame())
    and the land cells filled (cells_to_grid()).  keep (N,): the ocean cells; cell_index: the grid point of every cell
    of the arrays that place() takes.  sdims, coords and keep are those of the result."""

    def __init__(self, keep, cell_index, point, sdims, sshape, coords):
        self.point, self.cell_index, self.sshape = point, cell_index, tuple(sshape)
        self.C = int(np.asarray(keep, dtype=bool).sum())
        if point:
            self.sdims, self.coords, self.keep = (), {}, np.array(True)
        else:
            self.N = int(np.prod(self.sshape, dtype=np.int64))
            self.alive, self.coords, self.keep = grid_frame(np.asarray(keep, dtype=bool), sdims, self.sshape, coords)
            self.sdims = tuple(sdims)

    def place(self, a, fill, dtype):
        """(..., C) values of the cells as (..., *grid) of ``dtype``, ``fill`` on land"""
        a = np.asarray(a)
        if self.point:
            return a[..., 0].astype(dtype)
        return cells_to_grid(a, self.cell_index, self.N, self.sshape, self.alive, fill, dtype)


def grid_frame(keep, sdims, sshape, coords):
    """(alive, out_coords, keep on the grid) for per-cell results that go back on the grid: grid lines without an ocean
    cell are dropped, as unstack('cell') does in detect()."""
    from .detect import _alive_axes, _compress_grid
    alive = _alive_axes(keep, sshape)
    out_coords = {d: np.asarray(coords[d])[m] for d, m in zip(sdims, alive) if d in coords}
    return alive, out_coords, _compress_grid(keep.reshape(sshape), alive, 0)


def cells_to_grid(a, cell_index, N, sshape, alive, fill, dtype):
    """(..., C) values of the cells at ``cell_index`` as (..., *grid) with ``fill`` elsewhere, the dead grid lines of
    grid_frame() dropped"""
    from .detect import _compress_grid
    full = np.full(a.shape[:-1] + (N,), fill, dtype=dtype)
    full[..., cell_index] = a
    return np.ascontiguousarray(_compress_grid(full.reshape(a.shape[:-1] + tuple(sshape)), alive, a.ndim - 1))
