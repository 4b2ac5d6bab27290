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
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .gridweights import quantise_weights, resolve_weights, weights_label     # (quantise_weights: imported from here too)
from .series_stage import (Accumulators, check_weighted_cells, dense_ids, grid_layout, regions_of_result,     # noqa: F401
                           run, run_cells, run_grid)               # (grid_layout: imported from here too)

CATEGORIES = ("moderate", "strong", "severe", "extreme", "event")
WEIGHT_ONE = 1 << 31            # the quantised value of the largest weight
MAX_REGIONS = 1024              # XMHW_COVERAGE_MAX_REGIONS (include/xmhw_amd.h)


def _check_cells(C, wq, region, R):
    return check_weighted_cells(C, wq, region, R, MAX_REGIONS, "mhw_coverage", "wq")


class _Accumulators(Accumulators):
    """One call's arguments and its (T, R, 5) int64 device accumulators, which every slab ADDS to whole: they are not
    sliced by column, and nothing is out of range."""

    def __init__(self, wq, region, R, minDuration, joinGaps, maxGap, coldSpells):
        super().__init__()
        self.wq, self.region, self.R = wq, region, R
        self.filter = (int(minDuration), int(bool(joinGaps)), int(maxGap))
        self.neg = int(bool(coldSpells))

    def begin(self, T, C):
        """T steps; wq and region hold C entries"""
        self.wq, self.region, self.R = _check_cells(C, self.wq, self.region, self.R)
        shape = (T, self.R, len(CATEGORIES))
        self.make(None, {"cells": (shape, np.int64), "area_q": (shape, np.int64)})
        for ptr in self.ptrs():
            self.h.memset(ptr, 0, 8 * int(np.prod(shape)))

    def add_slab(self, slab):
        """One slab (series_stage.Slab): its cells' weights and region ids, exceedance bits, then the reduction."""
        d_ts, T, n = slab.d_ts, slab.T, slab.n
        W = (T + 63) // 64
        with DeviceScope() as s:
            d_wq, d_reg = s.upload(slab.take(self.wq)), s.upload(slab.take(self.region))
            d_bits = s.alloc(8 * W * n)
            with as_xmhw_errors(also="Unsupported"):
                self.h.exceed_bits(d_ts.ptr, slab.isz, T, n, slab.ld, slab.th_ptr, slab.ldc, slab.D, slab.rows, self.neg,
                                   d_bits.ptr, n)
                self.h.coverage_accumulate(d_ts.ptr, slab.isz, T, n, slab.ld, slab.se_ptr, slab.th_ptr, slab.ldc, slab.rows,
                                           self.neg, d_bits.ptr, n, *self.filter, d_wq.ptr, d_reg.ptr, self.R, *self.ptrs())
            self.h.stream_sync(0)                       # the slab's buffers are freed on the way out


def coverage_cells(ts, seas, thresh, doy, doys, wq, region, R, minDuration=5, joinGaps=True, maxGap=2, coldSpells=False,
                   max_batch_bytes=64 << 30, pad=None):
    """The device stage for a dense (T, C) series (arguments as detect_front.detect_cells): wq (C,) int64
    quantised weights in [0, 2**31], region (C,) ids in [-1, R) (-1: the cell counts nowhere).
    Returns (cells, area_q), both int64 (T, R, 5), columns CATEGORIES.  Cells go through the device in batches
    below max_batch_bytes; the sums are integers, so the batch size does not change a single bit."""
    return run_cells(_Accumulators(wq, region, R, minDuration, joinGaps, maxGap, coldSpells), ts, seas, thresh, doy, doys,
                     lambda T, isz, D: T * (isz + 1) + T // 4 + 2 * D * 8 + 64, max_batch_bytes, pad)


def coverage_grid(stacked, anynans, seas, thresh, doy, doys, wq, region, R, minDuration=5, joinGaps=True, maxGap=2,
                  coldSpells=False, max_batch_bytes=None, clim_stacked=False, pad=None):
    """coverage_cells() for an UNCOMPACTED stacked host series (T, N), as detect_front.detect_grid: the land mask
    and the compaction run on the device slab by slab (series_stage.walk_grid).  wq / region have N entries (the whole
    grid) and are compacted by each slab's `keep`: the accumulators begin with the shape of the grid, not with the ocean
    cells.  Returns (cells, area_q, keep[N])."""
    out, keep = run_grid(_Accumulators(wq, region, R, minDuration, joinGaps, maxGap, coldSpells), stacked, anynans, seas,
                         thresh, doy, doys, lambda T, D: 6 * D * 8 + T // 4 + 64, max_batch_bytes, clim_stacked, pad,
                         begin_with=stacked.shape)
    return out + (keep,)


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
    return dense_ids(labels, MAX_REGIONS, who, "regions")     # candidates: the labels on the whole grid


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
    layout = grid_layout(temp, tdim)
    coords, _, dims, point, sdims, sshape, N = layout
    # weights and region labels on the whole grid, in stacked order
    wq, unit = quantise_weights(resolve_weights(weights, coords, dims, tdim, sdims, sshape, point))
    found, rid, Rc = region_ids(regions, dims, tdim, sdims, sshape, point, N, "mhw_coverage")
    got = []

    def on_cells(host_keep, ts, sec, thc, doy, doys, *options, **extra):
        keep = host_keep()
        got.extend((_compute or coverage_cells)(ts, sec, thc, doy, doys, wq[keep], rid[keep], Rc, *options, **extra))

    def on_grid(stacked, anynans_, sec, thc, doy, doys, *options, **extra):
        *out, keep = coverage_grid(stacked, anynans_, sec, thc, doy, doys, wq, rid, Rc, *options, **extra)
        got.extend(out)
        return keep

    mhw = run(temp, th, se, layout, tdim, on_cells, on_grid, maxPadLength, coldSpells, tstep, anynans, _compute,
              max_batch_bytes, minDuration, joinGaps, maxGap)
    cells, area = (np.asarray(a) for a in got)
    T = np.asarray(coords[tdim]).shape[0]
    if cells.shape != (T, Rc, len(CATEGORIES)) or area.shape != cells.shape:
        raise XmhwException(f"coverage stage returned {cells.shape}, expected {(T, Rc, len(CATEGORIES))}")
    sel, ncells, total_q, region = regions_of_result(np.asarray(mhw.keep, dtype=bool), rid, wq, found)
    if sel is not None:
        cells, area = cells[:, sel], area[:, sel]
    attrs = {"weights": weights_label(weights), "xmhw_parameters": mhw.attrs["xmhw_parameters"]}
    return CoverageDataset(np.asarray(coords[tdim]), region, np.ascontiguousarray(cells), np.ascontiguousarray(area),
                           total_q, ncells, unit, tdim=tdim, attrs=attrs)
