"""regrid(): first-order conservative (area-overlap) remapping between two rectilinear lat-lon grids -- the front-end
stage that brings two products onto one grid before a two-field stage (mhw_cooccurrence(), lag_correlation(),
mhw_composite(), index_regression() with a gridded predictor): OISST (ascending latitude, centres at x.125) onto an
ERA5-style grid (descending, centres at x.00), either onto a model's 1 degree grid.  coarsen() nests integer blocks of
one grid; this stage takes any two.  Its output is an ordinary series.  One pass over the UNCOMPACTED grid in time blocks
(csrc/kernels_regrid.hip, csrc/regrid_index.h).

The definition (include/xmhw_amd.h, "regrid()", states it for the C entries).  Rectilinear grids make the overlap of
the destination cell (J, I) with the source cell (j, i) a product, the overlap of row J with row j times the overlap of
column I with column i: the device sees two small CSR tables and no 2-D weight matrix.  The row table: row_first[my],
row_ptr[my + 1]; destination row J reads the source rows row_first[J] + r, r < row_ptr[J + 1] - row_ptr[J] (consecutive
in memory order, whichever way latitude runs), under the int32 weights ay[row_ptr[J] + r]; wy[J] is the row's full extent
in the same unit.  The column table col_first, col_ptr, ax, wx likewise; on a periodic source the column is
(col_first[I] + k) mod nx.  0 <= ay, ax <= 2**12, a run holds 64 entries at most, the weights of a run sum to its extent
at most, wy, wx <= 2**18.  For (t, J, I), over the pairs (r, k) with w = ay * ax > 0 whose sample is not NaN:
    xq = rint((float64(x) - x0) * 2**16)             (the fixed point of region_series(), in float64 as written)
    a pair with |x - x0| >= 2**7, or infinite, is left out of all sums and counted (n_range, per pair)
    n += 1, wsum += w, xsum += w * xq                 (exact integers: |xsum| <= 2**59)
The cell is VALID iff n >= 1 and wsum * 65536 >= a * wy[J] * wx[I], a an integer in [0, 65536]: the least covered share in
65536ths, equality counts as valid.  The value is x0 + (float64(xsum) / float64(wsum)) / 65536.0 in float64 as written,
rounded once to the sample type; an invalid cell is NaN.  Every sum is an integer sum: the result does not depend on
launch geometry, step chunks, time blocks or the path the kernel takes, and numpy reproduces every bit.

Host side here (bounds, overlap tables, coordinates, time blocks); device side behind regrid_grid().
"""
import numpy as np

from ._lib import hip, hip_regrid
from .device import DeviceScope, as_xmhw_errors, device_budget_bytes, is_packed, native_float
from .exception import XmhwException
from .series_stage import grid_layout

MAX_RUN = 64                    # XMHW_REGRID_MAX_RUN (include/xmhw_amd.h)
MAX_WEIGHT = 4096               # XMHW_REGRID_MAX_WEIGHT: u, the weight of the largest overlap of a run
MAX_EXTENT = 1 << 18            # XMHW_REGRID_MAX_EXTENT
BITS = 16                       # XMHW_REGION_SERIES_BITS
RANGE_BITS = 7                  # |x - offset| < 2**7
SHARE_ONE = 65536               # min_fraction is taken in 65536ths
MEASURES = ("sphere", "plane")
PERIOD = 360.0                  # degrees of longitude


# ---- bounds and overlap tables -----------------------------------------------------------------------

def _monotone(v, what, least):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 1 or v.size < least or not np.isfinite(v).all():
        raise XmhwException(f"{what} should be a 1-D array of {least} finite numbers and more, got shape {v.shape}")
    d = np.diff(v)
    if v.size > 1 and not ((d > 0).all() or (d < 0).all()):
        raise XmhwException(f"{what} should be strictly ascending or strictly descending")
    return v


def axis_bounds(centres, limits=None):
    """(n + 1,) float64 cell bounds of the n cell ``centres`` (ascending or descending): the midpoints of neighbouring
    centres, the two ends extended by half a step; ``limits`` = (lo, hi) clips them (latitude: (-90, 90)).  One centre
    alone has no step: it needs ``limits``, which are then its bounds."""
    c = _monotone(centres, "the cell centres", 1)
    if c.size == 1:
        if limits is None:
            raise XmhwException("one cell centre alone has no step: pass limits or explicit bounds")
        lo, hi = float(min(limits)), float(max(limits))
        return np.array([lo, hi], dtype=np.float64)
    mid = 0.5 * (c[:-1] + c[1:])
    b = np.concatenate([[c[0] - 0.5 * (c[1] - c[0])], mid, [c[-1] + 0.5 * (c[-1] - c[-2])]])
    if limits is not None:
        b = np.clip(b, float(min(limits)), float(max(limits)))
    return b


def _measured(bounds, measure):
    return np.sin(np.deg2rad(bounds)) if measure == "sphere" else bounds


def overlap_table(src_bounds, dst_bounds, measure="plane", period=None):
    """The CSR overlap table of one axis: (first (m,) int32, ptr (m + 1,) int32, weights int32, full (m,) int32).

    ``src_bounds`` (n + 1,) and ``dst_bounds`` (m + 1,): the cell bounds along the axis, each ascending or descending, in
    the memory order of its cells.  ``measure``: "plane" takes lengths, "sphere" differences of sin(latitude in degrees).
    ``period`` (longitude, with "plane"): the destination cells are reduced modulo the period against the source, whose
    cells may not span more than it; a run may then wrap, first + k taken mod n.  Destination run J reads the source
    cells first[J] + k in memory order; its weights are rint(u * overlap / the largest overlap of the run) with u = 4096,
    zeros at the ends of a run dropped; full[J] is the cell's whole extent in that unit: the sum of the weights where
    the cell lies inside the source (a cell covered in full reaches the share 1 exactly), the rounded extent, and the sum
    at least, where it does not.  u is lowered for a run whose extent would exceed 2**18 units.  A destination cell outside the source has an
    empty run.  A run of more than 64 cells raises: coarsen() first."""
    if measure not in MEASURES:
        raise XmhwException(f"measure should be one of {MEASURES}, got {measure!r}")
    if period is not None and measure != "plane":
        raise XmhwException("a periodic axis is measured as a plane: pass measure='plane' with period")
    s = _measured(_monotone(src_bounds, "src_bounds", 2), measure)
    d = _measured(_monotone(dst_bounds, "dst_bounds", 2), measure)
    slo, shi = np.minimum(s[:-1], s[1:]), np.maximum(s[:-1], s[1:])
    dlo, dhi = np.minimum(d[:-1], d[1:]), np.maximum(d[:-1], d[1:])
    n, m = slo.size, dlo.size
    if period is not None:
        period = float(period)
        origin = float(slo.min())
        if not period > 0 or float(shi.max()) - origin > period * (1 + 1e-12):
            raise XmhwException(f"the source cells span {float(shi.max()) - origin}, more than the period {period}")
        shift = np.floor((dlo - origin) / period) * period
        dlo, dhi = dlo - shift, dhi - shift
        # the source cells once more, a period further on, in the order that keeps a wrapping run consecutive
        ascending = n == 1 or s[1] > s[0]
        slo = np.concatenate([slo, slo + period] if ascending else [slo + period, slo])
        shi = np.concatenate([shi, shi + period] if ascending else [shi + period, shi])
    first, count, weights, full = np.zeros(m, np.int32), np.zeros(m, np.int64), [], np.zeros(m, np.int32)
    for J in range(m):
        ov = np.minimum(dhi[J], shi) - np.maximum(dlo[J], slo)
        hit = np.nonzero(ov > 0)[0]
        if hit.size == 0:
            continue
        e0, e1 = int(hit[0]), int(hit[-1]) + 1
        o = np.clip(ov[e0:e1], 0.0, None)
        extent = float(dhi[J] - dlo[J])
        u = MAX_WEIGHT
        while True:
            w = np.rint(u * o / o.max()).astype(np.int64)
            # a cell inside the source is covered in full by its run: its extent IS the sum of its weights
            inside = abs(float(o.sum()) - extent) <= 1e-9 * extent
            whole = int(w.sum()) if inside else max(int(np.rint(u * extent / o.max())), int(w.sum()))
            if whole <= MAX_EXTENT or u == 1:
                break
            u = max(1, min(u - 1, int(u * MAX_EXTENT / whole)))
        if whole > MAX_EXTENT:
            raise XmhwException(f"destination cell {J} is more than 2**18 times its largest overlap: coarsen() first")
        keep = np.nonzero(w)[0]
        e0, e1, w = e0 + int(keep[0]), e0 + int(keep[-1]) + 1, w[keep[0]:keep[-1] + 1]
        if e1 - e0 > MAX_RUN or (period is not None and e1 - e0 > n):
            raise XmhwException(f"destination cell {J} overlaps {e1 - e0} source cells along the axis, more than "
                                f"{min(MAX_RUN, n)}: coarsen() first")
        first[J], count[J], full[J] = e0 % n, e1 - e0, whole
        weights.append(w)
    ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    weights = np.concatenate(weights).astype(np.int32) if weights else np.zeros(0, np.int32)
    return first, ptr, weights, full


def check_share(min_fraction):
    """a = rint(min_fraction * 65536), the least covered share in 65536ths"""
    try:
        f = float(min_fraction)
    except (TypeError, ValueError):
        f = np.nan
    if not 0.0 <= f <= 1.0:
        raise XmhwException(f"min_fraction should be in [0, 1], got {min_fraction!r}")
    return int(np.rint(f * SHARE_ONE))


def check_table(table, m, n, periodic, what):
    """(first, ptr, weights, full) as int32 arrays, checked as the C entries check them"""
    try:
        first, ptr, w, full = (np.ascontiguousarray(v) for v in table)
    except (TypeError, ValueError):
        raise XmhwException(f"the {what} table should be (first, ptr, weights, full)") from None
    if any(v.dtype.kind not in "iu" or v.ndim != 1 for v in (first, ptr, w, full)):
        raise XmhwException(f"the {what} table should hold 1-D arrays of whole numbers")
    first, ptr, w, full = (v.astype(np.int64) for v in (first, ptr, w, full))
    if first.shape != (m,) or ptr.shape != (m + 1,) or full.shape != (m,) or ptr[0] != 0 or (np.diff(ptr) < 0).any() or \
            w.shape[0] != ptr[-1]:
        raise XmhwException(f"the {what} table should be first[{m}], ptr[{m + 1}] from 0 and non-decreasing, "
                            f"weights[ptr[-1]] and full[{m}]")
    cnt = np.diff(ptr)
    if (cnt > MAX_RUN).any():
        raise XmhwException(f"a {what} run holds {int(cnt.max())} entries, more than {MAX_RUN}: coarsen() first")
    if w.size and (w.min() < 0 or w.max() > MAX_WEIGHT):
        raise XmhwException(f"the {what} weights should lie in [0, {MAX_WEIGHT}]")
    sums = np.add.reduceat(np.append(w, 0), ptr[:-1]) * (cnt > 0) if m else np.zeros(0, np.int64)
    if (sums > full).any() or (full > MAX_EXTENT).any():
        raise XmhwException(f"the {what} weights of a run should sum to its extent at most, and the extent be <= 2**18")
    live = cnt > 0
    inside = ((first >= 0) & (first < n) & (cnt <= n)) if periodic else ((first >= 0) & (first + cnt <= n))
    if (live & ~inside).any():
        raise XmhwException(f"a {what} run leaves the source grid of {n}")
    return tuple(v.astype(np.int32) for v in (first, ptr, w, full))


# ---- the device stage --------------------------------------------------------------------------------

def check_stage_inputs(field, ny, nx, my, mx, rows, cols, periodic, x0, a):
    """What both stages (the device's and a stand-in) may rely on: the arguments checked as the C entries check them and
    in the layouts the device takes"""
    if is_packed(field):
        raise XmhwException("regrid does not read packed int16 views: pass decoded floats")
    field = np.ascontiguousarray(native_float(np.asarray(field)))
    ny, nx, my, mx = (int(v) for v in (ny, nx, my, mx))
    if ny < 1 or nx < 1 or ny * nx >= 2 ** 31 or my < 0 or mx < 0 or my * mx >= 2 ** 31:
        raise XmhwException(f"regrid handles grids of 1 to 2**31 - 1 points, got {ny} x {nx} -> {my} x {mx}")
    if field.ndim != 2 or field.shape[1] != ny * nx:
        raise XmhwException(f"the series should be (T, {ny * nx}) on the {ny} x {nx} grid, got {field.shape}")
    rows = check_table(rows, my, ny, False, "row")
    cols = check_table(cols, mx, nx, bool(periodic), "column")
    x0, a = float(x0), int(a)
    if not np.isfinite(x0):
        raise XmhwException(f"offset should be a finite number, got {x0}")
    if not 0 <= a <= SHARE_ONE:
        raise XmhwException(f"a should be in [0, {SHARE_ONE}], got {a}")
    return field, ny, nx, my, mx, rows, cols, int(bool(periodic)), x0, a


def regrid_grid(field, ny, nx, my, mx, rows, cols, periodic, x0, a, want=False, max_batch_bytes=None, block_steps=None):
    """The device stage.  ``field`` (T, ny * nx): the UNCOMPACTED host series, float32 or float64; ``rows`` =
    (row_first, row_ptr, ay, wy) and ``cols`` = (col_first, col_ptr, ax, wx), the tables of the definition.  Returns
    (out (T, my * mx) in the dtype of the series, wsum int64 and n int32 likewise or None without ``want``, n_range).
    The series goes through the device in time blocks below ``max_batch_bytes`` (or of ``block_steps`` steps): upload
    the source block, queue the kernel, download the destination block; the tables are uploaded by the first block and
    reused by the others.  Any split of the steps gives the same bits.  Out-of-range samples are counted, not refused,
    here."""
    field, ny, nx, my, mx, rows, cols, periodic, x0, a = check_stage_inputs(field, ny, nx, my, mx, rows, cols, periodic, x0, a)
    T, cells, N = field.shape[0], my * mx, ny * nx
    isz = field.dtype.itemsize
    out = np.full((T, cells), np.nan, dtype=field.dtype)
    wsum = np.zeros((T, cells), dtype=np.int64) if want else None
    n = np.zeros((T, cells), dtype=np.int32) if want else None
    if T == 0 or cells == 0:
        return out, wsum, n, 0
    h, hr = hip(), hip_regrid()
    if max_batch_bytes is None:
        max_batch_bytes = device_budget_bytes()
    if block_steps is not None and int(block_steps) < 1:
        raise XmhwException("block_steps should be >= 1")
    per_step = N * isz + cells * (isz + (12 if want else 0))
    steps = int(block_steps) if block_steps else int(max(1, int(max_batch_bytes) // max(per_step, 1)))
    with DeviceScope() as resident:
        d_range = resident.upload(np.zeros(1, dtype=np.int64))
        for t0 in range(0, T, steps):
            t1 = min(t0 + steps, T)
            count = t1 - t0
            with DeviceScope() as s:
                d_ts = s.upload(field[t0:t1])
                d_out = s.alloc(count * cells * isz)
                d_wsum = s.alloc(count * cells * 8) if want else None
                d_n = s.alloc(count * cells * 4) if want else None
                with as_xmhw_errors(also="Unsupported"):
                    hr.regrid(d_ts.ptr, isz, count, N, ny, nx, *rows, *cols, periodic, x0, a, d_out.ptr, cells,
                              d_wsum.ptr if want else 0, d_n.ptr if want else 0, d_range.ptr)
                h.stream_sync(0)
                out[t0:t1] = d_out.to_array((count, cells), field.dtype)
                if want:
                    wsum[t0:t1] = d_wsum.to_array((count, cells), np.int64)
                    n[t0:t1] = d_n.to_array((count, cells), np.int32)
        n_range = int(d_range.to_array((1,), np.int64)[0])
    return out, wsum, n, n_range


# ---- the result --------------------------------------------------------------------------------------

class RegridInfo:
    """What regrid() says about its result, as plain arrays.

    rows = (row_first, row_ptr, ay, wy) and cols = (col_first, col_ptr, ax, wx): the tables of the definition; sdims
    and the destination coords; periodic, measure, offset; a = the least covered share in 65536ths; n_range = 0 (the
    call raises otherwise); coverage float32 (T, my, mx) = wsum / (wy * wx), the share of the cell's extent that had a
    sample (NaN for a cell without extent) -- filled only with ``coverage=True``, else None -- with wsum int64 and n
    int32 beside it."""

    def __init__(self, rows, cols, sdims, coords, periodic, measure, offset, a, n_range, dtype, coverage=None, wsum=None,
                 n=None, tdim="time", time=None, attrs=None):
        self.rows, self.cols = tuple(np.asarray(v) for v in rows), tuple(np.asarray(v) for v in cols)
        self.sdims, self.coords = tuple(sdims), dict(coords)
        self.periodic, self.measure, self.offset, self.a = bool(periodic), measure, float(offset), int(a)
        self.n_range, self.dtype = int(n_range), np.dtype(dtype)
        self.coverage, self.wsum, self.n = coverage, wsum, n
        self.tdim, self.time, self.attrs = tdim, time, dict(attrs or {})

    def quantisation_bound(self, values, spread):
        """A bound on |result - the mean of the same samples as float64 under the UNQUANTISED overlaps|, like ``values``
        (the result, (..., my, mx)); ``spread`` (broadcast against it): max - min of the source samples under the cell.

        Per axis an integer weight is c * overlap + e with |e| <= 1/2 (one rounding; an end cell whose weight rounded to
        0 was dropped from the run: e = -c * overlap, |e| <= 1/2 as well, so a run counts two entries more).  A pair's
        weight ay * ax then differs from its share c_y c_x o_y o_x by eps = ay e_x + ax e_y - e_y e_x, and two
        weighted means of the same samples differ by at most spread * sum |eps| / wsum (write both with normalised
        weights around the mid-range: the normalised weights differ by 2 sum |eps| / wsum in all, the samples lie within
        spread / 2 of the mid-range).  With Sy = sum ay, Sx = sum ax, ky and kx the entries of the two runs plus two:
            sum |eps| <= (kx * Sy + ky * Sx) / 2 + ky * kx / 4
        To that come 2**-17, the half unit by which a sample's fixed point is off, and half an ulp of the output type at
        the value, its one rounding (the float64 finish adds less than 2**-44).  wsum is the result's where the call
        kept it (``coverage=True``), else the least a valid cell can have, a * wy * wx / 65536 (infinite for a = 0).
        NaN where the value is."""
        v = np.asarray(values)
        (_, rp, ay, wy), (_, cp, ax, wx) = self.rows, self.cols
        ky, kx = np.diff(rp).astype(np.float64) + 2, np.diff(cp).astype(np.float64) + 2
        Sy = np.add.reduceat(np.append(ay, 0).astype(np.float64), rp[:-1]) * (np.diff(rp) > 0)
        Sx = np.add.reduceat(np.append(ax, 0).astype(np.float64), cp[:-1]) * (np.diff(cp) > 0)
        eps = (kx[None] * Sy[:, None] + ky[:, None] * Sx[None]) / 2 + ky[:, None] * kx[None] / 4
        if self.wsum is not None:
            wsum = np.asarray(self.wsum, dtype=np.float64)
        else:
            wsum = self.a * wy[:, None].astype(np.float64) * wx[None].astype(np.float64) / SHARE_ONE
        with np.errstate(divide="ignore", invalid="ignore"):
            weight_term = np.asarray(spread, dtype=np.float64) * eps / wsum
        half_ulp = 0.5 * np.spacing(np.abs(v.astype(self.dtype))).astype(np.float64)
        return np.where(np.isnan(v), np.nan, 2.0 ** -(BITS + 1) + half_ulp + weight_term)

    def to_xarray(self):
        import xarray as xr
        names = ("first", "ptr", "weights", "full")
        data = {}
        for axis, table in (("row", self.rows), ("col", self.cols)):
            data.update({f"{axis}_{k}": ((f"{axis}_{k}_index",), np.asarray(v)) for k, v in zip(names, table)})
        coords = {d: self.coords[d] for d in self.sdims if d in self.coords}
        if self.coverage is not None:
            dims = (self.tdim,) + self.sdims
            data.update(coverage=(dims, self.coverage), wsum=(dims, self.wsum), n=(dims, self.n))
            if self.time is not None:
                coords[self.tdim] = self.time
        return xr.Dataset(data, coords=coords,
                          attrs=dict(self.attrs, periodic=int(self.periodic), measure=self.measure, offset=self.offset,
                                     min_share_65536ths=self.a, n_range=self.n_range))


# ---- the public function -----------------------------------------------------------------------------

def _like_coords(like, tdim):
    """{dim: 1-D coordinate} of a GridSeries, a DataArray or a dict"""
    from .api import _is_xarray
    if isinstance(like, dict):
        return {k: np.asarray(v) for k, v in like.items()}
    if _is_xarray(like):
        return {d: like[d].values for d in like.dims if d != tdim and d in like.coords}
    if hasattr(like, "coords") and hasattr(like, "dims"):
        return {d: np.asarray(like.coords[d]) for d in like.dims if d != tdim and d in like.coords}
    raise XmhwException(f"like should be a GridSeries, a DataArray or a dict of coordinates, got {type(like).__name__}")


def _numeric(c, what):
    c = np.asarray(c)
    if c.dtype.kind not in "fiu" or c.ndim != 1 or c.size < 1:
        raise XmhwException(f"{what} should be a 1-D numeric coordinate")
    return c.astype(np.float64)


def regrid(temp, like=None, lat=None, lon=None, lat_bounds=None, lon_bounds=None, src_lat_bounds=None, src_lon_bounds=None,
           periodic=None, measure="sphere", min_fraction=0.5, offset=0.0, coverage=False, tdim="time", max_batch_bytes=None,
           block_steps=None, _compute=None):
    """First-order conservative remapping of a series onto another rectilinear lat-lon grid.

    ``temp``: a GridSeries or an xarray.DataArray with two spatial dims in the stacked (sorted-name) order of
    landmask.stack_cells: the first is the latitude (rows), the second the longitude (columns, the fast axis), both with
    numeric coordinates; samples are read as stored, packed int16 views are refused.  The destination grid: ``like`` (a
    GridSeries, a DataArray or a dict {dim: centres} with the same two dim names), or ``lat`` and ``lon`` centres;
    ``lat_bounds`` / ``lon_bounds`` (m + 1 each) replace the bounds that axis_bounds() derives from the centres (then
    the centres may be left out: they are the midpoints), ``src_lat_bounds`` / ``src_lon_bounds`` those of the source.
    Either axis of either grid may ascend or descend.  ``periodic``: the source longitude closes on itself; None = it
    does when its bounds span 360 degrees.  Destination longitudes are then reduced modulo 360 against the source:
    -180..180 and 0..360 name the same cells.  ``measure``: "sphere" weighs latitude by differences of sin(lat),
    "plane" by lengths; longitude is always a length.  ``min_fraction`` in [0, 1]: the least share of a destination
    cell's extent (land and the part outside the source included) that must have had a sample, taken in 65536ths,
    a = rint(min_fraction * 65536); a cell at exactly that share is valid.  ``offset``: x0 of the definition;
    |temp - offset| must stay below 2**7 (``offset=273.15`` for kelvin), else the call raises.  A destination cell may
    overlap 64 source cells per axis at most: coarsen() first for more.

    Returns ``(series, info)``: ``series`` has the type, the dims, the dim order, the floating dtype (other dtypes
    become float64) and the attrs of the input, with the destination coordinates.  ``info`` is a RegridInfo;
    ``coverage=True`` fills its coverage, wsum and n.  ``block_steps``: the steps of a time block on the device (None:
    what fits ``max_batch_bytes``); blocks change no bit.  ``_compute``: a stand-in for regrid_grid() (host tests)."""
    from .api import GridSeries, _is_xarray
    from .landmask import stack_cells
    if measure not in MEASURES:
        raise XmhwException(f"measure should be one of {MEASURES}, got {measure!r}")
    a = check_share(min_fraction)
    offset = float(offset)
    if not np.isfinite(offset):
        raise XmhwException(f"offset should be a finite number, got {offset}")
    coords, _, dims, point, sdims, sshape, N = grid_layout(temp, tdim)
    if point or len(sdims) != 2:
        raise XmhwException(f"regrid needs two spatial dims (latitude, longitude), got {list(sdims)}")
    values = temp.values
    if is_packed(values):
        raise XmhwException("regrid does not read packed int16 views: pass decoded floats")
    ydim, xdim = sdims
    ny, nx = (int(v) for v in sshape)
    # the source bounds
    sy = np.asarray(src_lat_bounds, np.float64) if src_lat_bounds is not None else \
        axis_bounds(_numeric(coords[ydim], f"the {ydim} coordinate"), (-90.0, 90.0) if measure == "sphere" else None)
    sx = np.asarray(src_lon_bounds, np.float64) if src_lon_bounds is not None else \
        axis_bounds(_numeric(coords[xdim], f"the {xdim} coordinate"))
    if sy.shape != (ny + 1,) or sx.shape != (nx + 1,):
        raise XmhwException(f"the source bounds should hold {ny + 1} and {nx + 1} values, got {sy.shape} and {sx.shape}")
    # the destination centres and bounds
    given = _like_coords(like, tdim) if like is not None else {}
    if like is not None and (lat is not None or lon is not None):
        raise XmhwException("pass like or lat / lon, not both")
    if like is not None and not (ydim in given and xdim in given):
        raise XmhwException(f"like should carry the coordinates {ydim!r} and {xdim!r} of the series, got {sorted(given)}")
    dlat, dlon = (given.get(ydim), given.get(xdim)) if like is not None else (lat, lon)
    dst = {}
    for d, centres, bounds, limits in ((ydim, dlat, lat_bounds, (-90.0, 90.0) if measure == "sphere" else None),
                                       (xdim, dlon, lon_bounds, None)):
        if bounds is not None:
            b = _monotone(bounds, f"the destination bounds of {d}", 2)
            c = 0.5 * (b[:-1] + b[1:]) if centres is None else _numeric(centres, f"the destination {d}")
            if c.shape != (b.size - 1,):
                raise XmhwException(f"the destination bounds of {d} should hold one value more than its centres")
        elif centres is not None:
            c = _numeric(centres, f"the destination {d}")
            b = axis_bounds(c, limits)
        else:
            raise XmhwException(f"no destination grid along {d}: pass like, or lat and lon, or their bounds")
        dst[d] = (c, b)
    if periodic is None:
        periodic = abs(abs(float(sx[-1] - sx[0])) - PERIOD) <= 1e-6 * PERIOD
    rows = overlap_table(sy, dst[ydim][1], measure)
    cols = overlap_table(sx, dst[xdim][1], "plane", PERIOD if periodic else None)
    my, mx = dst[ydim][0].size, dst[xdim][0].size
    field = stack_cells(np.asarray(values), dims, tdim)[0]
    stage = _compute or regrid_grid
    out, wsum, n, n_range = stage(field, ny, nx, my, mx, rows, cols, int(bool(periodic)), offset, a, want=bool(coverage),
                                  max_batch_bytes=max_batch_bytes, block_steps=block_steps)
    T = field.shape[0]
    out = np.asarray(out)
    if out.shape != (T, my * mx):
        raise XmhwException(f"regrid stage returned {out.shape}, expected {(T, my * mx)}")
    if n_range:
        raise XmhwException(f"{int(n_range)} (destination, source) pairs hold samples 2**{RANGE_BITS} and more from "
                            f"offset={offset} (or infinite): pass offset=273.15 for a series in kelvin")
    new_coords = {tdim: np.asarray(coords[tdim]), ydim: dst[ydim][0], xdim: dst[xdim][0]}
    order_now = [tdim, ydim, xdim]
    grid = np.transpose(out.reshape(T, my, mx), [order_now.index(d) for d in dims])
    cov = None
    if coverage:
        whole = rows[3][:, None].astype(np.float64) * cols[3][None].astype(np.float64)
        wsum, n = np.asarray(wsum).reshape(T, my, mx), np.asarray(n).reshape(T, my, mx)
        with np.errstate(divide="ignore", invalid="ignore"):
            cov = (wsum.astype(np.float64) / whole[None]).astype(np.float32)
    info = RegridInfo(rows, cols, sdims, {ydim: new_coords[ydim], xdim: new_coords[xdim]}, periodic, measure, offset, a,
                      n_range, out.dtype, cov, wsum if coverage else None, n if coverage else None, tdim, new_coords[tdim])
    if _is_xarray(temp):
        import xarray as xr
        xc = {tdim: temp[tdim]} if tdim in temp.coords else {}
        xc.update({d: xr.Variable((d,), new_coords[d], attrs=dict(temp[d].attrs) if d in temp.coords else {}) for d in sdims})
        series = xr.DataArray(grid, dims=temp.dims, coords=xc, attrs=dict(temp.attrs), name=temp.name)
    else:
        series = GridSeries(grid, temp.dims, {d: new_coords[d] for d in dims if d in new_coords}, attrs=temp.attrs,
                            coord_attrs=temp.coord_attrs, time_encoding=temp.time_encoding)
    return series, info
