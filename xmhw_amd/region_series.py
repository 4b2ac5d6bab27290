"""region_series(): the area-weighted mean series of every region -- the box, basin or EEZ average that most
marine-heatwave case studies (and every Nino-style index) start from.  Average the SST over the region, then run
threshold() and detect() on that one series.  The series stays on the device: the sum across cells is one streaming
pass (csrc/kernels_region.hip), and only (time, region) numbers come back.

The definition.  For a step t and a region r, over the ocean cells c of r whose sample is not NaN:
    n_valid (int64) = their number,        wsum_i (int64) = sum wi[c],
    xsum_q (int64)  = sum wi[c] * xq[t, c],    xq = rint((float64(ts[t, c]) - offset) * 2**16)   (SERIES_BITS = 16),
xq in float64 exactly as written: the product by 2**16 is exact and rint rounds half to even, so
``numpy.rint((ts.astype(float64) - offset) * 65536.0)`` is the same integer for every sample, and all sums are
integer sums: exact, and independent of the order of the adds, of the slabs and of the launch geometry.
A valid sample with |ts - offset| >= 2**7, or infinite, is left out of every sum and counted, and the call raises:
no value outside the stated bound ever reaches a sum.  Pass ``offset=273.15`` for a series in kelvin.

The bit budget (that of track_intensity.intensity_bits).  wi = rint(w / w.max() * 2**ib), ib = min(31, 61 - 16 - 7 -
bit_length(C_ocean)), C_ocean = the ocean cells of the WHOLE grid.  A step of a region holds at most C_ocean samples,
wi <= 2**ib and |xq| <= 2**23, so |xsum_q| <= C_ocean * 2**(ib + 23) < 2**61 whatever the data.  A grid that leaves
fewer than 2 bits is refused (with ib = 1 the weights would be 0, 1 or 2: no weighting at all; ib < 1 has no budget).

Derived on the host, in float64: mean = offset + xsum_q / (wsum_i * 2**16) (NaN where wsum_i == 0) and
valid_fraction = wsum_i / total_i, the share of the region's weight that had a sample.

Host side here (validation, weights, region labels, slabs); device side behind region_cells() (a dense host series) and
region_grid() (a stacked grid, masked and compacted on the device slab by slab).
"""
import numpy as np

from ._lib import hip
from .api import GridSeries, _is_xarray
from .coverage import region_ids
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .gridweights import quantise_weights, resolve_weights, weights_label
from .series_stage import check_weighted_cells, grid_layout, regions_of_result

SERIES_BITS = 16                # XMHW_REGION_SERIES_BITS (include/xmhw_amd.h)
RANGE_BITS = 7                  # |ts - offset| < 2**7
MAX_REGIONS = 1024              # XMHW_REGION_MAX_REGIONS
MAX_WEIGHT_BITS = 31
FIELDS = ("n_valid", "wsum_i", "xsum_q")


def weight_bits(n_ocean):
    """ib of the module docstring; raises for a grid that leaves fewer than 2 bits"""
    ib = int(min(MAX_WEIGHT_BITS, 61 - SERIES_BITS - RANGE_BITS - int(n_ocean).bit_length()))
    if ib < 2:
        raise XmhwException(f"a grid with {int(n_ocean)} ocean cells leaves no bits for the weights of region_series()")
    return ib


def _check_cells(C, wi, region, R, offset):
    wi, region, R = check_weighted_cells(C, wi, region, R, MAX_REGIONS, "region_series", "wi")
    offset = float(offset)
    if not np.isfinite(offset):
        raise XmhwException(f"offset should be a finite number, got {offset}")
    return wi, region, R, offset


class _Accumulators:
    """The (T, R, 3) int64 device accumulator and the range counter, zeroed; read back once at the end."""

    def __init__(self, h, T, R):
        self.h, self.shape = h, (T, R, len(FIELDS))
        self._scope = DeviceScope()
        self.nbytes = 8 * T * R * len(FIELDS)
        self.acc, self.n_range = self._scope.alloc(max(self.nbytes, 8)), self._scope.alloc(8)
        h.memset(self.acc.ptr, 0, max(self.nbytes, 8))
        h.memset(self.n_range.ptr, 0, 8)

    def add_slab(self, d_ts, isz, T, n, ld, offset, wi, region, R):
        """a slab of n cells whose series is on the device: upload its weights and region ids, queue the pass"""
        with DeviceScope() as s:
            d_wi, d_reg = s.upload(wi), s.upload(region)
            with as_xmhw_errors(also="Unsupported"):
                self.h.region_accumulate(d_ts.ptr, isz, T, n, ld, offset, d_wi.ptr, d_reg.ptr, R, self.acc.ptr, self.n_range.ptr)
            self.h.stream_sync(0)                       # d_wi / d_reg are freed on the way out

    def result(self):
        self.h.stream_sync(0)
        acc = self.acc.to_array(self.shape, np.int64) if self.nbytes else np.zeros(self.shape, np.int64)
        return acc, int(self.n_range.to_array((1,), np.int64)[0])

    def free(self):
        self._scope.free()


def region_cells(ts, wi, region, R, offset=0.0, max_batch_bytes=64 << 30):
    """The device stage for a dense host (T, C) series: wi (C,) int64 weights in [0, 2**31], region (C,) ids in
    [-1, R) (-1: the cell counts nowhere), offset the float64 x0.  Returns (acc int64 (T, R, 3) with columns FIELDS,
    n_range).  Cells go through the device in batches below max_batch_bytes; the sums are integers, so the batch
    size does not change a single bit."""
    from .device import native_float
    ts = np.asarray(native_float(ts))
    if ts.ndim != 2:
        raise XmhwException("ts should be a (time, cells) array")
    T, C = ts.shape
    wi, region, R, offset = _check_cells(C, wi, region, R, offset)
    h = hip()
    isz = ts.dtype.itemsize
    batch = int(max(1, min(max(C, 1), max_batch_bytes // max(T * isz + 16, 1))))
    acc = _Accumulators(h, T, R)
    try:
        for c0 in range(0, C, batch):
            n = min(C, c0 + batch) - c0
            with DeviceScope() as s:
                d_ts = s.upload(np.ascontiguousarray(ts[:, c0:c0 + n]))
                acc.add_slab(d_ts, isz, T, n, n, offset, wi[c0:c0 + n], region[c0:c0 + n], R)
        return acc.result()
    finally:
        acc.free()


def region_grid(stacked, anynans, wi_of, region, R, offset=0.0, max_batch_bytes=None):
    """region_cells() for an UNCOMPACTED stacked host series (T, N), float or a packed int16 / big-endian file view:
    the land mask and the compaction run on the device slab by slab, as in coverage_grid().  ``region`` (N,) holds the
    ids of the whole grid; ``wi_of(C_ocean)`` returns its (N,) int64 weights once the ocean cells are counted (ib
    depends on their number).  A grid that fits one slab is uploaded once: masked, counted, compacted, summed.  A larger
    one takes a first pass that uploads every slab for its land mask alone, then the pass that compacts and sums:
    the series crosses the bus twice, and no host copy of it is ever read.  Returns (acc, n_range, keep[N])."""
    from .device import (SlabPrefetcher, _grid_batch, device_itemsize, is_packed, mask_compact, native_float)
    if not is_packed(stacked):
        stacked = np.ascontiguousarray(native_float(stacked))
    T, N = stacked.shape
    region = np.ascontiguousarray(region, dtype=np.int32)
    if region.shape != (N,):
        raise XmhwException("region should have one entry per cell")
    _check_cells(0, np.zeros(0, np.int64), np.zeros(0, np.int32), R, offset)
    h = hip()
    isz = device_itemsize(stacked)
    cb = _grid_batch(stacked, max_batch_bytes, per_cell_extra=16)
    slabs = [(lo, min(N, lo + cb)) for lo in range(0, N, cb)]
    first = []                                          # per slab: (compacted buffer or None, keep)
    held = DeviceScope()
    try:
        pre = SlabPrefetcher(stacked, slabs)
        try:
            for (lo, hi), (d_up, up_isz) in pre:
                d_ts, keep = mask_compact(d_up, up_isz, T, hi - lo, anynans)
                if len(slabs) == 1:
                    held.adopt(d_ts)                    # the one slab stays for the sums
                elif d_ts is not None:
                    d_ts.free()
                    d_ts = None
                first.append((d_ts, keep))
        finally:
            pre.close()
        keep = np.concatenate([k for _, k in first]) if first else np.zeros(0, dtype=bool)
        if not keep.any():
            raise XmhwException("All points of grid are either land or NaN")
        wi = np.ascontiguousarray(wi_of(int(keep.sum())), dtype=np.int64)
        wi, region, R, offset = _check_cells(N, wi, region, R, offset)
        acc = _Accumulators(h, T, R)
        try:
            if len(slabs) == 1:
                n = int(keep.sum())
                acc.add_slab(first[0][0], isz, T, n, n, offset, wi[keep], region[keep], R)
            else:
                pre = SlabPrefetcher(stacked, slabs)
                try:
                    for i, ((lo, hi), (d_up, up_isz)) in enumerate(pre):
                        d_ts, again = mask_compact(d_up, up_isz, T, hi - lo, anynans)
                        with DeviceScope() as s:
                            s.adopt(d_ts)
                            if not np.array_equal(again, first[i][1]):
                                raise XmhwException("the series changed between the two passes of region_series()")
                            if d_ts is None:
                                continue
                            n = int(again.sum())
                            acc.add_slab(d_ts, isz, T, n, n, offset, wi[lo:hi][again], region[lo:hi][again], R)
                finally:
                    pre.close()
            got, n_range = acc.result()
        finally:
            acc.free()
        return got, n_range, keep
    finally:
        held.free()


class RegionSeriesDataset:
    """What region_series() returns, as plain arrays.

    time (T,), region (R,) the region labels (sorted; [0] without ``regions``);
    n_valid, wsum_i, xsum_q   int64 (T, R): the sums of the module docstring;
    ncells, total_i (R,)      the number and the integer weight of the region's ocean cells;
    weight_bits (ib), weight_unit = w.max() / 2**ib (``wsum_i * weight_unit`` is in the units of the weights), offset;
    mean (T, R) float64       offset + xsum_q / (wsum_i * 2**16), NaN where wsum_i == 0;
    valid_fraction (T, R)     wsum_i / total_i (NaN for a region without ocean weight)."""

    def __init__(self, time, region, n_valid, wsum_i, xsum_q, ncells, total_i, weight_bits, weight_unit, offset, tdim="time",
                 attrs=None, series_attrs=None, time_encoding=None, time_attrs=None):
        self.time, self.region = np.asarray(time), np.asarray(region)
        self.n_valid, self.wsum_i, self.xsum_q = n_valid, wsum_i, xsum_q
        self.ncells, self.total_i = ncells, total_i
        self.weight_bits, self.weight_unit, self.offset = int(weight_bits), float(weight_unit), float(offset)
        self.tdim, self.attrs, self.series_attrs = tdim, dict(attrs or {}), dict(series_attrs or {})
        self.time_encoding, self.time_attrs = dict(time_encoding or {}), dict(time_attrs or {})
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = self.offset + xsum_q.astype(np.float64) / (wsum_i.astype(np.float64) * 2.0 ** SERIES_BITS)
            frac = wsum_i.astype(np.float64) / total_i.astype(np.float64)[None, :]
        self.mean = np.where(wsum_i > 0, mean, np.nan)
        frac[:, total_i == 0] = np.nan
        self.valid_fraction = frac

    def quantisation_bound(self):
        """(T, R) float64: a bound on |mean - sum(w x) / sum(w)| over the valid samples of every entry, for the
        unquantised float64 weights w and the samples x as float64.  The derivation of
        TrackIntensityDataset.quantisation_bound() carried over, with a = x - offset in (-2**7, 2**7): the rounding of
        aq = 2**16 a + r, |r| <= 1/2, moves the weighted mean by at most 2**-17; the rounding of the weights, wi = s w +
        d, |d| <= 1/2, moves it by sum(d (a - mu)) / sum(wi) with |a - mu| < 2**8, below n_valid * 2**7 / wsum_i; the
        float64 evaluation (two conversions, a division of a value below 2**7 and the add of the offset) adds less than
        2**-44.  NaN where wsum_i == 0."""
        with np.errstate(divide="ignore", invalid="ignore"):
            b = self.n_valid.astype(np.float64) * 2.0 ** RANGE_BITS / self.wsum_i.astype(np.float64)
        return np.where(self.wsum_i > 0, b + 2.0 ** -(SERIES_BITS + 1) + 2.0 ** -44, np.nan)

    def series(self, min_fraction=0.0):
        """The regional means as a GridSeries with dims (tdim, "region") that threshold(), detect() and
        threshold_detect() take: ``mean``, NaN where valid_fraction < min_fraction.  It carries the input's
        time_encoding and attrs."""
        min_fraction = float(min_fraction)
        if not 0.0 <= min_fraction <= 1.0:
            raise XmhwException(f"min_fraction should be in [0, 1], got {min_fraction}")
        with np.errstate(invalid="ignore"):
            values = np.where(self.valid_fraction < min_fraction, np.nan, self.mean)
        return GridSeries(values, (self.tdim, "region"), {self.tdim: self.time, "region": self.region},
                          attrs=self.series_attrs, coord_attrs={self.tdim: self.time_attrs},
                          time_encoding=self.time_encoding)

    def to_xarray(self):
        import xarray as xr
        dims = (self.tdim, "region")
        data = {k: (dims, getattr(self, k)) for k in FIELDS + ("mean", "valid_fraction")}
        data["ncells"], data["total_i"] = (("region",), self.ncells), (("region",), self.total_i)
        return xr.Dataset(data, coords={self.tdim: self.time, "region": self.region},
                          attrs=dict(self.attrs, weight_bits=self.weight_bits, weight_unit=self.weight_unit, offset=self.offset,
                                     series_bits=SERIES_BITS))


def region_series(temp, weights=None, regions=None, tdim="time", offset=0.0, anynans=False, max_batch_bytes=None,
                  _compute=None):
    """The area-weighted mean series of every region of a temperature grid.

    ``temp``: a GridSeries, an xarray.DataArray or a single-point (time-only) series.  ``weights`` and ``regions`` mean
    and validate what they do in mhw_coverage() (same exceptions): None, "coslat" or an array on the spatial grid,
    finite, >= 0, not all zero; None or an integer array on the spatial grid, negative = the cell counts nowhere, at
    most 1024 labels.  The regions of the result are the sorted non-negative labels found on ocean cells; land is
    what land_check() drops (all-NaN cells; any-NaN with ``anynans``).  ``offset``: subtracted before the fixed-point
    conversion and added back to the mean; |temp - offset| must stay below 2**7 (``offset=273.15`` for kelvin).

    Returns a RegionSeriesDataset (module docstring: the definition; class docstring: the fields); its ``series()``
    goes straight into threshold() / detect() / threshold_detect().  Every integer is a sum of integers: exact, and the
    same from run to run and for every ``max_batch_bytes``.  ``_compute``: a stand-in for region_cells() (host tests)."""
    from . import landmask
    coords, _, dims, point, sdims, sshape, N = grid_layout(temp, tdim)
    w = resolve_weights(weights, coords, dims, tdim, sdims, sshape, point)
    quantise_weights(w)                                        # the checks of mhw_coverage(), before anything else
    found, rid, Rc = region_ids(regions, dims, tdim, sdims, sshape, point, N, "region_series")
    offset = float(offset)
    if not np.isfinite(offset):
        raise XmhwException(f"offset should be a finite number, got {offset}")
    wi_of = lambda n_ocean: quantise_weights(w, weight_bits(n_ocean))[0]      # noqa: E731
    values = temp.values
    time = np.asarray(coords[tdim])
    T = time.shape[0]
    if point:
        keep = np.array([True])
        wi = wi_of(1)
        stage = _compute or region_cells
        acc, n_range = stage(np.ascontiguousarray(np.asarray(values).reshape(-1, 1)), wi, rid, Rc, offset)
    elif _compute is not None:
        ts, keep, _, _ = landmask.land_check(np.asarray(values), dims, tdim, anynans)
        wi = wi_of(int(keep.sum()))
        acc, n_range = _compute(ts, wi[keep], rid[keep], Rc, offset)
    else:
        stacked, _, _ = landmask.stack_cells(values, dims, tdim)
        acc, n_range, keep = region_grid(stacked, anynans, wi_of, rid, Rc, offset, max_batch_bytes=max_batch_bytes)
        wi = wi_of(int(keep.sum()))
    acc = np.asarray(acc)
    if acc.shape != (T, Rc, len(FIELDS)):
        raise XmhwException(f"region stage returned {acc.shape}, expected {(T, Rc, len(FIELDS))}")
    if n_range:
        raise XmhwException(f"{int(n_range)} samples lie 2**{RANGE_BITS} and more from offset={offset} (or are infinite): "
                            "pass offset=273.15 for a series in kelvin")
    ib = weight_bits(int(keep.sum()))
    sel, ncells, total_i, region = regions_of_result(keep, rid, wi, found)
    if sel is not None:
        acc = acc[:, sel]
    if _is_xarray(temp):
        enc, tattrs = dict(getattr(temp[tdim], "encoding", {}) or {}), dict(temp[tdim].attrs)
        sattrs = dict(temp.attrs)
    else:
        enc, tattrs, sattrs = temp.time_encoding, temp.coord_attrs.get(tdim, {}), temp.attrs
    attrs = {"weights": weights_label(weights)}
    n_valid, wsum_i, xsum_q = (np.ascontiguousarray(acc[:, :, k]) for k in range(len(FIELDS)))
    return RegionSeriesDataset(time, region, n_valid, wsum_i, xsum_q, ncells, total_i, ib, float(w.max()) / (1 << ib), offset,
                               tdim=tdim, attrs=attrs, series_attrs=sattrs, time_encoding=enc, time_attrs=tattrs)
