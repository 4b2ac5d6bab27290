"""mhw_coverage(): the daily area in each MHW category, by region -- the reduction ACROSS cells that
every user of a gridded detect() takes next (Hobday et al. 2018, fig. 3: the share of the ocean, of a basin,
of an EEZ that is in a Moderate / Strong / Severe / Extreme heatwave on each day).  Not in xmhw nor in
marineHeatWaves; the semantics are those of detect():

* a step of a cell is *in an event* iff detect() labels it (mhw_filter() + join_gaps(), gap steps of joined
  events included);
* its category is the per-step one of mhw_df() (xmhw/features.py:52-66):
  ``cats = floor(1 + (ts - thresh) / (thresh - seas))`` in float64, moderate / strong / severe / extreme =
  ``cats == 1``, ``== 2``, ``== 3``, ``>= 4``.  A gap step (below the threshold, or NaN) is in none of the four.

Outputs are int64 (T, R, 5), columns CATEGORIES: ``cells`` counts cells, ``area_q`` sums their weights.

Weights are fixed point.  The float weights w (>= 0) are quantised once on the host, ``wq = rint(w / w.max() *
2**31)``, and all sums are integer sums: exact, and independent of the order of the adds, of the slab size and
of the launch geometry.  ``fraction = area_q / total_q``.  Distance from the unquantised ratio: with
u = w.max() / 2**31 (``weight_unit``) every ``wq * u`` is within u/2 of its w, so a numerator A = sum of w
over n_s cells and the denominator B = sum of w over the region's n ocean cells (n_s <= n) are reproduced
within n_s u/2 and n u/2.  For 0 <= A <= B and B' > 0:

    |A'/B' - A/B| = |(A' - A) B - A (B' - B)| / (B B') <= (n_s + n) u / (2 B') <= n u / B'

(A <= B was used for the second term).  quantisation_bound() returns ``ncells * weight_unit / (total_q *
weight_unit) = ncells / total_q`` per region; the host test asserts it against math.fsum.

Host side here (validation, weights, region labels, slabs); device side in csrc/kernels_coverage.hip.
"""
import numpy as np

from . import gridweights
from ._lib import hip
from .api import GridSeries, _from_xarray, _is_xarray
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .gridweights import quantise_weights, resolve_weights, weights_label     # (quantise_weights: imported from here too)

CATEGORIES = ("moderate", "strong", "severe", "extreme", "event")
WEIGHT_ONE = 1 << 31            # the quantised value of the largest weight
MAX_REGIONS = 1024              # XMHW_COVERAGE_MAX_REGIONS (include/xmhw_amd.h)


def _check_cells(C, wq, region, R):
    wq = np.ascontiguousarray(wq, dtype=np.int64)
    region = np.ascontiguousarray(region, dtype=np.int32)
    if wq.shape != (C,) or region.shape != (C,):
        raise XmhwException("wq and region should have one entry per cell")
    if C and (wq.min() < 0 or wq.max() > WEIGHT_ONE):
        raise XmhwException("quantised weights should be in [0, 2**31]")
    R = int(R)
    if R < 1:
        raise XmhwException("R should be >= 1")
    if C and (region.min() < -1 or region.max() >= R):
        raise XmhwException("region ids should be in [-1, R)")
    if R > MAX_REGIONS:
        raise XmhwException(f"mhw_coverage handles at most {MAX_REGIONS} regions, got {R}")
    return wq, region, R


def _accumulate_device(h, d_ts, isz, se_ptr, th_ptr, ldc, D, rows, T, n, neg, minDuration, joinGaps, maxGap, d_wq, d_reg,
                       R, d_cells, d_area, ld=None):
    """One slab of n cells already on the device (series d_ts, leading dimension ld; climatologies at their
    column offset, leading dimension ldc): exceedance bits, then the reduction ADDS into d_cells / d_area."""
    ld = n if ld is None else ld
    W = (T + 63) // 64
    with DeviceScope() as s:
        d_bits = s.alloc(8 * W * n)
        with as_xmhw_errors(also="Unsupported"):
            h.exceed_bits(d_ts.ptr, isz, T, n, ld, th_ptr, ldc, D, rows, neg, d_bits.ptr, n)
            h.coverage_accumulate(d_ts.ptr, isz, T, n, ld, se_ptr, th_ptr, ldc, rows, neg, d_bits.ptr, n, int(minDuration),
                                  int(bool(joinGaps)), int(maxGap), d_wq.ptr, d_reg.ptr, R, d_cells.ptr, d_area.ptr)
        h.stream_sync(0)                                # d_bits is freed on the way out


class _Accumulators:
    """The (T, R, 5) int64 device accumulators, zeroed; read back once at the end."""

    def __init__(self, h, T, R):
        self.h, self.shape = h, (T, R, len(CATEGORIES))
        nbytes = 8 * T * R * len(CATEGORIES)
        self._scope = DeviceScope()
        self.cells, self.area = self._scope.alloc(nbytes), self._scope.alloc(nbytes)
        h.memset(self.cells.ptr, 0, nbytes)
        h.memset(self.area.ptr, 0, nbytes)

    def result(self):
        self.h.stream_sync(0)
        return self.cells.to_array(self.shape, np.int64), self.area.to_array(self.shape, np.int64)

    def free(self):
        self._scope.free()


def coverage_cells(ts, seas, thresh, doy, doys, wq, region, R, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False,
                   max_batch_bytes=64 << 30, pad=None):
    """The device stage for a dense (T, C) series (arguments as detect_front.detect_cells): wq (C,) int64
    quantised weights in [0, 2**31], region (C,) ids in [-1, R) (-1: the cell counts nowhere).
    Returns (cells, area_q), both int64 (T, R, 5), columns CATEGORIES.  Cells go through the device in batches
    below max_batch_bytes; the sums are integers, so the batch size does not change a single bit."""
    from .detect_front import _check_inputs
    ts, seas, thresh, rows = _check_inputs(ts, seas, thresh, doy, doys)
    T, C = ts.shape
    D = thresh.shape[0]
    wq, region, R = _check_cells(C, wq, region, R)
    h = hip()
    isz = ts.dtype.itemsize
    neg = int(bool(coldSpells))
    per_cell = T * (isz + 1) + T // 4 + 2 * D * 8 + 64
    batch = int(max(1, min(C, max_batch_bytes // max(per_cell, 1))))
    acc = _Accumulators(h, T, R)
    try:
        for c0 in range(0, C, batch):
            c1 = min(C, c0 + batch)
            n = c1 - c0
            with DeviceScope() as s:
                d_ts = s.upload(np.ascontiguousarray(ts[:, c0:c1]))
                if pad is not None:
                    pad.apply(d_ts.ptr, isz, T, n)
                d_se = s.upload(np.ascontiguousarray(seas[:, c0:c1]))
                d_th = s.upload(np.ascontiguousarray(thresh[:, c0:c1]))
                d_wq, d_reg = s.upload(wq[c0:c1]), s.upload(region[c0:c1])
                _accumulate_device(h, d_ts, isz, d_se.ptr, d_th.ptr, n, D, rows, T, n, neg, minDuration, joinGaps, maxGap,
                                   d_wq, d_reg, R, acc.cells, acc.area)
        return acc.result()
    finally:
        acc.free()


def coverage_grid(stacked, anynans, seas, thresh, doy, doys, wq, region, R, minDuration=5, joinGaps=True, maxGap=2,
                  coldSpells=False, max_batch_bytes=None, clim_stacked=False, pad=None):
    """coverage_cells() for an UNCOMPACTED stacked host series (T, N), as detect_front.detect_grid: the land mask
    and the compaction run on the device slab by slab, the climatologies are compacted there as well
    (clim_stacked) and pair up with the series' survivors by position.  wq / region have N entries (the whole
    grid) and are compacted by each slab's `keep`.  Returns (cells, area_q, keep[N])."""
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
    wq, region, R = _check_cells(N, wq, region, R)
    h = hip()
    isz = device_itemsize(stacked)
    neg = int(bool(coldSpells))
    keeps = []
    acc = _Accumulators(h, T, R)
    clim = DeviceScope()
    k0 = 0
    try:
        if clim_stacked:
            d_th, keep_th = compact_columns(thresh, 0, thresh.shape[1], anynans)
            clim.adopt(d_th)
            d_se, keep_se = compact_columns(seas, 0, seas.shape[1], anynans)
            clim.adopt(d_se)
            C, Cse = int(keep_th.sum()), int(keep_se.sum())
            if C == 0 or Cse == 0:
                raise XmhwException("All points of grid are either land or NaN")
        else:
            d_th, d_se = clim.upload(thresh), clim.upload(seas)
            C, Cse = thresh.shape[1], seas.shape[1]
        if C != Cse:
            raise XmhwException(f"th and se do not have the same ocean cells: {C}, {Cse}")
        cb = _grid_batch(stacked, max_batch_bytes, per_cell_extra=6 * D * 8 + T // 4 + 64)
        for lo in range(0, N, cb):
            hi = min(N, lo + cb)
            d_ts, keep = compact_columns(stacked, lo, hi, anynans)
            keeps.append(keep)
            n = int(keep.sum())
            if d_ts is None:
                continue
            with DeviceScope() as s:
                s.adopt(d_ts)
                if pad is not None:
                    pad.apply(d_ts.ptr, isz, T, n)
                if k0 + n > C:
                    raise XmhwException(f"temp has more ocean cells than th and se ({C})")
                d_wq, d_reg = s.upload(wq[lo:hi][keep]), s.upload(region[lo:hi][keep])
                _accumulate_device(h, d_ts, isz, d_se.ptr + 8 * k0, d_th.ptr + 8 * k0, C, D, rows, T, n, neg, minDuration,
                                   joinGaps, maxGap, d_wq, d_reg, R, acc.cells, acc.area)
            k0 += n
        keep = np.concatenate(keeps) if keeps else np.zeros(0, dtype=bool)
        if not keep.any():
            raise XmhwException("All points of grid are either land or NaN")
        if k0 != C:
            raise XmhwException(f"temp has {k0} ocean cells, th and se have {C}")
        cells, area = acc.result()
        return cells, area, keep
    finally:
        acc.free()
        clim.free()


class CoverageDataset:
    """What mhw_coverage() returns, as plain arrays.

    time (T,), region (R,) the region labels (sorted; [0] without `regions`), category = CATEGORIES;
    cells, area_q  int64 (T, R, 5): the number of cells in each state and the sum of their quantised weights;
    fraction       float64 (T, R, 5) = area_q / total_q (NaN for a region without ocean weight);
    total_q, ncells (R,): the quantised weight and the number of the region's ocean cells;
    weight_unit    w.max() / 2**31: ``area_q * weight_unit`` is an area in the units of the weights."""

    def __init__(self, time, region, cells, area_q, total_q, ncells, weight_unit, tdim="time", attrs=None):
        self.time, self.region, self.category = np.asarray(time), np.asarray(region), CATEGORIES
        self.cells, self.area_q = cells, area_q
        self.total_q, self.ncells, self.weight_unit = total_q, ncells, float(weight_unit)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = area_q.astype(np.float64) / total_q.astype(np.float64)[None, :, None]
        frac[:, total_q == 0, :] = np.nan
        self.fraction = frac

    def quantisation_bound(self):
        """(R,) bound on |fraction - sum(w [state]) / sum(w)| from the quantisation alone (module docstring)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.total_q > 0, self.ncells / self.total_q.astype(np.float64), np.nan)

    def to_xarray(self):
        import xarray as xr
        dims = (self.tdim, "region", "category")
        return xr.Dataset(
            {"cells": (dims, self.cells), "area_q": (dims, self.area_q), "fraction": (dims, self.fraction),
             "total_q": (("region",), self.total_q), "ncells": (("region",), self.ncells)},
            coords={self.tdim: self.time, "region": self.region, "category": list(CATEGORIES)},
            attrs=dict(self.attrs, weight_unit=self.weight_unit))


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


def region_ids(regions, dims, tdim, sdims, sshape, point, N, who):
    """The ``regions`` argument on the whole grid, in stacked order: (found, rid, Rc) with ``found`` the sorted
    non-negative labels, ``rid`` (N,) int32 the position of every cell's label in it (-1: negative label, the cell
    counts nowhere) and Rc = max(len(found), 1).  ``who`` names the caller in the message of the cap."""
    if regions is None:
        labels = np.zeros(N, dtype=np.int64)
    else:
        regions = np.asarray(regions)
        if regions.dtype.kind not in "iu":
            raise XmhwException(f"regions should be an integer array, got {regions.dtype}")
        labels = regions.astype(np.int64).reshape(-1) if point else \
            gridweights.on_grid(regions, "regions", dims, tdim, sdims, sshape).astype(np.int64)
        if labels.shape != (N,):
            raise XmhwException("regions should have one entry per cell")
    found = np.unique(labels[labels >= 0])                     # candidates: the labels on the whole grid
    rid = np.where(labels >= 0, np.searchsorted(found, labels), -1).astype(np.int32)
    Rc = max(int(found.shape[0]), 1)
    if Rc > MAX_REGIONS:
        raise XmhwException(f"{who} handles at most {MAX_REGIONS} regions, got {Rc}")
    return found, rid, Rc


def mhw_coverage(temp, th, se, weights=None, regions=None, tdim="time", minDuration=5, joinGaps=True, maxGap=2,
                 maxPadLength=None, coldSpells=False, tstep=False, anynans=False, _compute=None, max_batch_bytes=None):
    """Daily count and weighted area of the cells in each MHW category, by region.

    ``temp``, ``th``, ``se`` and the options shared with detect() mean and validate what they do there (same
    exceptions, land masking and positional pairing of series and climatology cells).
    ``weights``: None (1 per cell), "coslat" (cos of the latitude coordinate) or an array on the spatial grid
    (the non-time dims of ``temp``, in its order): finite, >= 0, not all zero.  They are quantised to
    ``rint(w / w.max() * 2**31)`` (w.max() over the whole grid) and summed as integers.
    ``regions``: None (one region) or an integer array on the spatial grid; negative = the cell counts nowhere.
    The regions of the result are the sorted non-negative labels found on ocean cells.
    A single-point series gives R = 1.

    Returns a CoverageDataset: cells / area_q int64 (time, region, 5) with columns moderate, strong, severe,
    extreme, event (event >= the sum of the four: gap days of joined events are in none of them), ``fraction =
    area_q / total_q`` within ``quantisation_bound()`` of the unquantised ratio.  ``_compute``: a stand-in for
    coverage_cells() (host tests)."""
    from .detect import _detect
    coords, coord_attrs, dims, point, sdims, sshape, N = grid_layout(temp, tdim)
    # weights and region labels on the whole grid, in stacked order
    wq, unit = quantise_weights(resolve_weights(weights, coords, dims, tdim, sdims, sshape, point))
    found, rid, Rc = region_ids(regions, dims, tdim, sdims, sshape, point, N, "mhw_coverage")
    got = {}

    def on_cells(ts, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, intermediate, pad=None):
        # _detect() has masked and compacted on the host (point series, or a stand-in device stage)
        from .landmask import keep_mask, stack_cells
        if point:
            keep = np.array([True])
        else:
            vals = temp.values
            keep = keep_mask(stack_cells(np.asarray(vals), dims, tdim)[0], anynans)
        stage = _compute or coverage_cells
        extra = {} if pad is None else {"pad": pad}
        if max_batch_bytes is not None and _compute is None:
            extra["max_batch_bytes"] = max_batch_bytes
        got["cells"], got["area"] = stage(ts, sec, thc, doy, doys, wq[keep], rid[keep], Rc, minDuration, joinGaps, maxGap,
                                          coldSpells, **extra)
        return dict(table=np.zeros((0, 31)), offsets=np.zeros(ts.shape[1] + 1, dtype=np.int64), inter=None)

    def on_grid(stacked, anynans_, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells, intermediate,
                clim_stacked=False, pad=None):
        got["cells"], got["area"], keep = coverage_grid(stacked, anynans_, sec, thc, doy, doys, wq, rid, Rc, minDuration,
                                                        joinGaps, maxGap, coldSpells, max_batch_bytes=max_batch_bytes,
                                                        clim_stacked=clim_stacked, pad=pad)
        return dict(table=np.zeros((0, 31)), offsets=np.zeros(int(keep.sum()) + 1, dtype=np.int64), inter=None, keep=keep)

    series = GridSeries(temp.values, dims, coords, coord_attrs=coord_attrs) if _is_xarray(temp) else temp
    as_series = lambda a: GridSeries(a.values, a.dims, _from_xarray(a)[0]) if _is_xarray(a) else a   # noqa: E731
    mhw = _detect(series, as_series(th), as_series(se), on_cells, tdim, minDuration, joinGaps, maxGap, maxPadLength,
                  coldSpells, False, anynans, tstep, grid_compute=None if _compute is not None else on_grid)
    keep = np.asarray(mhw.keep, dtype=bool)
    cells, area = np.asarray(got["cells"]), np.asarray(got["area"])
    T = np.asarray(coords[tdim]).shape[0]
    if cells.shape != (T, Rc, len(CATEGORIES)) or area.shape != cells.shape:
        raise XmhwException(f"coverage stage returned {cells.shape}, expected {(T, Rc, len(CATEGORIES))}")
    # the regions of the result: the labels found on OCEAN cells
    ocean = keep & (rid >= 0)
    ncells = np.bincount(rid[ocean], minlength=Rc).astype(np.int64)
    total_q = np.zeros(Rc, dtype=np.int64)
    np.add.at(total_q, rid[ocean], wq[ocean])
    if found.shape[0]:
        sel = ncells > 0
        cells, area, ncells, total_q, region = cells[:, sel], area[:, sel], ncells[sel], total_q[sel], found[sel]
    else:
        region = np.zeros(1, dtype=np.int64)                    # every cell excluded: one empty region
    attrs = {"weights": weights_label(weights), "xmhw_parameters": mhw.attrs["xmhw_parameters"]}
    return CoverageDataset(np.asarray(coords[tdim]), region, np.ascontiguousarray(cells), np.ascontiguousarray(area),
                           total_q, ncells, unit, tdim=tdim, attrs=attrs)
