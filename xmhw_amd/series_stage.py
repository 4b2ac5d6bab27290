"""What the stages that read the series and the climatologies together share ("What 3.7, 3.11 and 3.16
share"): mhw_coverage(), mhw_track_intensity() and mhw_days_by() reduce them over the event steps, and each is a slab
method on top of the things that exist once, here:

* Slab                      one slab of cells on the device, as the slab methods take it;
* climatologies_on_device() seas / thresh whole on the device, compacted there if needed (detect_grid() uses it too);
* walk_cells(), walk_grid() the dense and the grid slab walker;
* run()                     the one shim around detect._detect();
* dense_ids(), check_class_ids(), check_weighted_cells()    labels and the stage-side checks of per-cell arguments;
* regions_of_result()       the regions found on ocean cells (mhw_coverage(), region_series());
* walk_stage(), report_range()      one stage call around its accumulators, and its out-of-range count (mhw_days_by(),
                            heat_stress());
* CellFrame, grid_frame(), cells_to_grid()      per-cell results back on the grid (mhw_days_by(), mhw_cooccurrence(),
                            mhw_displacement(), heat_stress());
* grid_layout()             the spatial layout of a GridSeries / DataArray.
"""
from collections import namedtuple

import numpy as np

from .api import GridSeries, _from_xarray, _is_xarray
from .device import DeviceScope
from .exception import XmhwException

LAND_TEXT = "All points of grid are either land or NaN"


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
        from .landmask import keep_mask, stack_cells
        if point:
            return np.array([True])
        return keep_mask(stack_cells(np.asarray(temp.values), dims, tdim)[0], anynans)

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


def report_range(n_range, counters, text):
    """What a stage does with its count of samples outside the fixed-point range: into ``counters`` (a dict) when the
    caller collects it, otherwise an exception worded by ``text``."""
    if counters is not None:
        counters["n_range"] = int(n_range)
    elif n_range:
        raise XmhwException(f"{int(n_range)} {text}")


def walk_stage(acc, walker, text, counters):
    """One stage call around its accumulators (begin(), add_slab(), result() -> (arrays, n_range), free()):
    ``walker(acc)`` sends the slabs through them and returns keep[N] or None; the accumulators are freed whatever
    happens, then the range count is reported.  Returns (arrays, keep)."""
    try:
        keep = walker(acc)
        out, n_range = acc.result()
    finally:
        acc.free()
    report_range(n_range, counters, text)
    return out, keep


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
