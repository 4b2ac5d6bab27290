"""mhw_displacement(): the thermal displacement (Jacox et al. 2020, "Thermal displacement by marine heatwaves", Nature
584) of every MHW cell-day -- for a cell in a heatwave on a given day, the distance to the nearest place whose SST that
day is no warmer than what the heatwave cell would normally have: how far an organism would have to move to stay at its
usual temperature.  Every other stage after detect() reduces a cell's own series, or follows the neighbours an event
table names; this is the first one whose cells look at the temperature FIELD around them: a data-dependent search over
the resident grid, one day at a time (csrc/kernels_displacement.hip).

The definition (results are exact integers).  The grid has one latitude and one longitude dim with 1-D coordinates,
longitude the fast axis of the stacked layout and uniformly spaced: dlon = (lon[-1] - lon[0]) / (nx - 1), every spacing
within 1e-6 of it, relative; latitude may be irregular.  For a source at grid row j, column i and a destination (j', i'):
    dj = j' - j,  di = i' - i, or with ``periodic``: di = (i' - i) mod nx, minus nx if that exceeds nx // 2,
and in float64, with phi = radians(lat) and dlam = radians(di * dlon):
    h       = sin^2((phi' - phi) / 2) + cos phi cos phi' sin^2(dlam / 2), clipped to [0, 1]
    dist_m  = int(rint(1000 * radius * 2 * asin(sqrt(h))))
    north_m = int(rint(1000 * radius * (phi' - phi)))
    east_m  = int(rint(1000 * radius * cos((phi + phi') / 2) * dlam))     the MID-LATITUDE zonal component
all functions of (j, dj, di) alone (pair_metrics()).  displacement_offsets() lists, per grid row j, every (dj, di) with
0 <= j + dj < ny, di admissible and dist_m <= rint(1000 * max_distance), sorted ascending by (dist_m, dj, di): the first
entry is (0, 0).

A SOURCE is a cell-day (c, t) in an event of ``mhw``: some table row of cell c has index_start <= t <= index_end (gap
days of joined events included; the rasteriser event_table_bits of mhw_cooccurrence(), over all ocean cells).  A source
whose ``basin`` label is negative is skipped and counted nowhere.  With x(t, p) = float64(temp[t, p]), negated under
coldSpells, the target of a source is its own climatology g = seas[row(t), c], and a grid point p = (j + dj, i + di)
QUALIFIES iff x(t, p) is not NaN (land is NaN in the uncompacted grid), x(t, p) <= g and, with a ``basin``,
basin[p] == basin[source].  A p outside a grid without wrap does not qualify; a source with NaN g finds nothing; the
source itself is candidate 0 (on a gap day with x <= seas the displacement is 0).  The result of a source is the first
qualifying entry of its row's list -- the minimum of (dist_m, dj, di) over all qualifying points within reach -- or
the source is unreached.

Per class k of time steps (``classes``, as in mhw_days_by(); label -1 counts nowhere) and ocean cell c:
    n_days int32 the sources, n_found int32 those reached, sum_m / sum_north_m / sum_east_m int64 the sums over the found
    sources, max_m int32 the largest dist_m found (0 if none); dist_m < 2**25 and at most 2**31 steps: no overflow.
Per call, n_visited: the sum over the sources of the list entries that source alone had to look at (the position found
plus one, or the whole list length; entries outside the grid included).  Everything is an integer sum or maximum: the
result does not depend on the time blocks, the launch geometry or the schedule.

Samples are read AS STORED: ``maxPadLength`` is refused (a destination is never an interpolated value), packed int16
views are refused (pass decoded floats), and a grid point that is land to detect() but holds a value on some day is a
destination on that day.  Not in this version: per-event or per-object displacement and the destination of every
cell-day (open ends).

Host side here (grid and table, validation, time blocks, the dataset); device side behind displacement_grid().
"""
from collections import namedtuple

import numpy as np

from ._lib import hip
from .device import DeviceScope, as_xmhw_errors, device_budget_bytes, is_packed, native_float
from .exception import XmhwException
from .series_stage import (LAND_TEXT, CellFrame, check_class_ids, check_view, class_labels, climatologies_on_device, dense_ids,
                           grid_layout, run)

MAX_CLASSES = 1024              # XMHW_DISPLACEMENT_MAX_CLASSES (include/xmhw_amd.h)
MAX_AXIS = 32767                # XMHW_DISPLACEMENT_MAX_AXIS: dj and di travel as int16
DIST_BITS = 25                  # dist_m < 2**25
EARTH_RADIUS_KM = 6371.0
STAGE_FIELDS = ("n_days", "n_found", "sum_m", "sum_north_m", "sum_east_m", "max_m")
_STAGE = dict(n_days=np.int32, n_found=np.int32, sum_m=np.int64, sum_north_m=np.int64, sum_east_m=np.int64, max_m=np.int32)
LAT_NAMES, LON_NAMES = ("lat", "latitude"), ("lon", "longitude")
_COLD_TEXT = "cold events were detected"
_TABLE_ENTRY_BYTES = 16         # packed (dj, di) + dist_m + north_m + east_m


def pair_metrics(phi, phi2, dlam, radius=EARTH_RADIUS_KM):
    """(dist_m, north_m, east_m) int64 of the pairs with latitudes ``phi`` -> ``phi2`` and longitude difference ``dlam``
    (radians, float64, broadcast against each other): THE per-pair function of the module docstring -- the table and
    the brute-force oracle of the tests both call it, elementwise, so they agree to the last metre."""
    phi, phi2, dlam = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (phi, phi2, dlam)))
    h = np.sin((phi2 - phi) / 2.0) ** 2 + np.cos(phi) * np.cos(phi2) * np.sin(dlam / 2.0) ** 2
    h = np.clip(h, 0.0, 1.0)
    scale = 1000.0 * float(radius)
    dist = np.rint(scale * 2.0 * np.arcsin(np.sqrt(h))).astype(np.int64)
    north = np.rint(scale * (phi2 - phi)).astype(np.int64)
    east = np.rint(scale * np.cos((phi + phi2) / 2.0) * dlam).astype(np.int64)
    return dist, north, east


def di_range(nx, periodic):
    """The admissible di, ascending: -(nx - 1) .. nx - 1 without wrap; with wrap the nx values nx // 2 - nx + 1 ..
    nx // 2 (each destination column exactly once)."""
    nx = int(nx)
    if periodic:
        return np.arange(nx // 2 - nx + 1, nx // 2 + 1, dtype=np.int64)
    return np.arange(-(nx - 1), nx, dtype=np.int64)


def wrapped_di(i_src, i_dst, nx, periodic):
    """di from column i_src to column i_dst (arrays broadcast)"""
    d = np.asarray(i_dst, dtype=np.int64) - np.asarray(i_src, dtype=np.int64)
    if periodic:
        d = d % nx
        d = np.where(d > nx // 2, d - nx, d)
    return d


class DisplacementTable:
    """What displacement_offsets() returns: the geometry (lat (ny,) degrees, nx, dlon degrees, max_distance km, periodic,
    radius km, max_m = rint(1000 * max_distance)) and the candidate lists as CSR: row_offsets (ny + 1,) int64, djdi
    (E, 2) int16 -- the packed (dj, di) stream -- and dist_m, north_m, east_m (E,) int32.  row(j) gives the five slices
    of grid row j."""

    def __init__(self, lat, nx, dlon, max_distance, periodic, radius, row_offsets, djdi, dist_m, north_m, east_m):
        self.lat, self.nx, self.dlon = np.asarray(lat, dtype=np.float64), int(nx), float(dlon)
        self.ny = int(self.lat.shape[0])
        self.max_distance, self.periodic, self.radius = float(max_distance), bool(periodic), float(radius)
        self.max_m = int(np.rint(1000.0 * self.max_distance))
        self.row_offsets, self.djdi, self.dist_m, self.north_m, self.east_m = row_offsets, djdi, dist_m, north_m, east_m

    @property
    def n_entries(self):
        return int(self.row_offsets[-1])

    @property
    def nbytes(self):
        return _TABLE_ENTRY_BYTES * self.n_entries + 8 * (self.ny + 1)

    def row(self, j):
        sl = slice(int(self.row_offsets[j]), int(self.row_offsets[j + 1]))
        return self.djdi[sl, 0], self.djdi[sl, 1], self.dist_m[sl], self.north_m[sl], self.east_m[sl]

    def packed(self):
        """the (dj, di) stream as the device takes it: int32, dj << 16 | di & 0xFFFF"""
        return ((self.djdi[:, 0].astype(np.int32) << 16) | (self.djdi[:, 1].astype(np.int32) & 0xFFFF)).astype(np.int32)


def _check_geometry(lat, nx, dlon, max_distance, radius):
    lat = np.asarray(lat, dtype=np.float64)
    if lat.ndim != 1 or lat.shape[0] < 1 or not np.isfinite(lat).all() or np.abs(lat).max() > 90.0:
        raise XmhwException("latitude should be a 1-D array of finite degrees in [-90, 90]")
    nx = int(nx)
    if nx < 1:
        raise XmhwException("nx should be >= 1")
    if lat.shape[0] > MAX_AXIS or nx > MAX_AXIS:
        raise XmhwException(f"mhw_displacement handles grid axes of at most {MAX_AXIS} points, got {lat.shape[0]} x {nx}")
    if not np.isfinite(dlon) or (nx > 1 and dlon == 0.0):
        raise XmhwException(f"dlon should be finite and non-zero, got {dlon}")
    if not (np.isfinite(max_distance) and max_distance >= 0.0):
        raise XmhwException(f"max_distance should be a distance in km >= 0, got {max_distance}")
    if not (np.isfinite(radius) and radius > 0.0):
        raise XmhwException(f"radius should be a positive length in km, got {radius}")
    if 1000.0 * radius * np.pi >= float(1 << DIST_BITS):
        raise XmhwException(f"radius {radius} km: half a great circle does not stay below 2**{DIST_BITS} m")
    return lat, nx


def displacement_offsets(lat, nx, dlon, max_distance=1000.0, periodic=False, radius=EARTH_RADIUS_KM, max_table_bytes=None):
    """The candidate lists of a grid: ``lat`` (ny,) the latitudes in degrees, ``nx`` columns ``dlon`` degrees apart,
    ``max_distance`` and ``radius`` in km, ``periodic``: longitude wraps.  Per grid row j the list of all (dj, di) with
    0 <= j + dj < ny, di in di_range(nx, periodic) and dist_m <= rint(1000 * max_distance), sorted ascending by the key
    (dist_m, dj, di); the first entry is always (0, 0).  Returns a DisplacementTable.  A table above ``max_table_bytes``
    is refused (None: no limit)."""
    lat, nx = _check_geometry(lat, nx, dlon, max_distance, radius)
    ny = lat.shape[0]
    periodic = bool(periodic)
    max_m = int(np.rint(1000.0 * float(max_distance)))
    scale = 1000.0 * float(radius)
    phi = np.deg2rad(lat)
    di_all = di_range(nx, periodic)
    dlam_all = np.deg2rad(di_all.astype(np.float64) * float(dlon))
    sl2 = np.sin(dlam_all / 2.0) ** 2
    # what cannot be in a list is cut before the exact evaluation, with slack far above the rounding of either side:
    # the great-circle distance is at least the meridional one, and h <= sin^2(reach / 2) bounds sin^2(dlam / 2)
    reach = (max_m + 2.0) / scale
    hmax = np.sin(min(reach, np.pi) / 2.0) ** 2 * (1.0 + 1e-9) + 1e-15
    parts, offsets, total = [], np.zeros(ny + 1, dtype=np.int64), 0
    for j in range(ny):
        rows = np.nonzero(np.abs(phi - phi[j]) <= reach)[0]
        a = np.sin((phi[rows] - phi[j]) / 2.0) ** 2
        b = np.cos(phi[j]) * np.cos(phi[rows])
        near = (a[:, None] + b[:, None] * sl2[None, :]) <= hmax
        r, d = np.nonzero(near)
        dist, north, east = pair_metrics(phi[j], phi[rows[r]], dlam_all[d], radius)
        ok = dist <= max_m
        dj, di, dist, north, east = (rows[r] - j)[ok], di_all[d][ok], dist[ok], north[ok], east[ok]
        order = np.lexsort((di, dj, dist))
        parts.append((dj[order], di[order], dist[order], north[order], east[order]))
        total += order.shape[0]
        offsets[j + 1] = total
        if max_table_bytes is not None and _TABLE_ENTRY_BYTES * total > max_table_bytes:
            raise XmhwException(f"the candidate lists of max_distance={max_distance} km need more than {max_table_bytes} "
                                f"bytes on the device (row {j} of {ny} reached): lower max_distance")
    cat = lambda k, dtype: np.ascontiguousarray(np.concatenate([p[k] for p in parts]), dtype=dtype)      # noqa: E731
    djdi = np.ascontiguousarray(np.stack([cat(0, np.int16), cat(1, np.int16)], axis=1))
    return DisplacementTable(lat, nx, dlon, max_distance, periodic, radius, offsets, djdi, cat(2, np.int32),
                             cat(3, np.int32), cat(4, np.int32))


def _check_basin(basin, N):
    """None, or the labels as (N,) int32"""
    if basin is None:
        return None
    basin = np.asarray(basin)
    if basin.dtype.kind not in "iu" or basin.size != N:
        raise XmhwException(f"basin should hold one integer label per grid point ({N}), got {basin.dtype} {basin.shape}")
    if basin.size and (basin.min() < -(1 << 31) or basin.max() >= (1 << 31)):
        raise XmhwException("basin labels should fit int32")
    return np.ascontiguousarray(basin.reshape(N), dtype=np.int32)


class DeviceSeas(namedtuple("DeviceSeas", "ptr ld D C")):
    """seas (D, C) float64 already on the device: pointer, leading dimension, rows, ocean cells"""
    __slots__ = ()
    ndim = 2

    @property
    def shape(self):
        return (self.D, self.C)


def check_stage_inputs(field, seas, rows, view, cell_index, table, classes, K, basin):
    """What both stages (the device's and a stand-in) may rely on: returns (field, rows, cell_of_point, classes, K,
    basin) checked and in the layouts the device takes."""
    if is_packed(field):
        raise XmhwException("mhw_displacement does not read packed int16 views: pass decoded floats")
    field = native_float(np.asarray(field))
    ny, nx = table.ny, table.nx
    N = ny * nx
    if field.ndim != 2 or field.shape[1] != N:
        raise XmhwException(f"the series should be (T, {N}) on the {ny} x {nx} grid of the table, got {field.shape}")
    T = field.shape[0]
    if T < 1:
        raise XmhwException("the series has no time step")
    cell_index = np.ascontiguousarray(cell_index, dtype=np.int64)
    C = cell_index.shape[0]
    if seas.ndim != 2 or seas.shape[1] != C:
        raise XmhwException(f"seas should be (D, {C}) on the ocean cells, got {seas.shape}")
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.shape != (T,) or (rows.min() < 0 or rows.max() >= seas.shape[0]):
        raise XmhwException("rows should hold the climatology row of every time step")
    if view["C"] != C:
        raise XmhwException(f"the event table has {view['C']} cells, the grid {C} ocean cells: mhw does not belong to temp")
    check_view(view, np.arange(C, dtype=np.int64), T, "mhw")
    if C and (cell_index.min() < 0 or cell_index.max() >= N or (np.diff(cell_index) <= 0).any()):
        raise XmhwException("cell_index should hold ascending grid points")
    cell_of_point = np.full(N, -1, dtype=np.int32)
    cell_of_point[cell_index] = np.arange(C, dtype=np.int32)
    classes, K = check_class_ids(T, classes, K, MAX_CLASSES, "mhw_displacement")
    basin = _check_basin(basin, N)
    return field, rows, cell_of_point, classes, K, basin


class _Accumulators:
    """One call's device state: the bitmap of the event table, the maps, the candidate lists and the accumulators stay
    resident; add_block() ADDS a block of steps; result() reads back once."""

    def __init__(self, view, cell_of_point, table, classes, K, basin, coldSpells, T, rows):
        self.h, self.table, self.classes, self.K, self.T, self.rows = hip(), table, classes, int(K), int(T), rows
        self.neg = int(bool(coldSpells))
        self.C = C = int(view["C"])
        self._scope = s = DeviceScope()
        try:
            n = max(self.K * C, 1)
            self.out32 = [s.alloc(4 * n) for _ in range(3)]            # n_days, n_found, max_m
            self.out64 = [s.alloc(8 * n) for _ in range(3)]            # sum_m, sum_north_m, sum_east_m
            self.count = s.alloc(8)
            with as_xmhw_errors(also="Unsupported"):
                self.h.displacement_init(self.K, C, *self._out())
            W = (self.T + 63) // 64
            self.bits = s.alloc(8 * W * max(C, 1))
            with DeviceScope() as tmp:
                some = view["n"] > 0
                d_start = tmp.upload(view["start"] if some else np.zeros(1, np.int32))
                d_end = tmp.upload(view["end"] if some else np.zeros(1, np.int32))
                d_off, d_cell = tmp.upload(view["offsets"]), tmp.upload(np.arange(max(C, 1), dtype=np.int64))
                with as_xmhw_errors(also="Unsupported"):
                    self.h.event_table_bits(d_start.ptr, d_end.ptr, d_off.ptr, d_cell.ptr, C, self.T, self.bits.ptr, C)
                self.h.stream_sync(0)                   # the table's buffers are freed on the way out
            self.cell_of_point = s.upload(cell_of_point)
            self.basin = s.upload(basin) if basin is not None else None
            E = table.n_entries
            self.list_off = s.upload(table.row_offsets)
            self.djdi, self.dist, self.north, self.east = (s.upload(a if E else np.zeros(1, np.int32)) for a in
                                                           (table.packed(), table.dist_m, table.north_m, table.east_m))
        except BaseException:
            s.free()
            raise

    def _out(self):
        n_days, n_found, max_m = (b.ptr for b in self.out32)
        return (n_days, n_found) + tuple(b.ptr for b in self.out64) + (max_m, self.C, self.count.ptr)

    def add_block(self, ts_ptr, isz, ld, t0, nt, se_ptr, ldc, D):
        """the steps t0 .. t0 + nt - 1: their uncompacted rows are at ts_ptr, leading dimension ld >= ny * nx"""
        t = self.table
        with as_xmhw_errors(also="Unsupported"):
            self.h.displacement_accumulate(ts_ptr, isz, ld, t0, nt, self.T, t.ny, t.nx, int(t.periodic), se_ptr, ldc, D,
                                           self.rows, self.neg, self.bits.ptr, self.C, self.cell_of_point.ptr, self.C,
                                           self.basin.ptr if self.basin is not None else 0, self.list_off.ptr,
                                           self.djdi.ptr, self.dist.ptr, self.north.ptr, self.east.ptr, t.n_entries,
                                           self.classes, self.K, *self._out())

    def result(self):
        K, C = self.K, self.C
        self.h.stream_sync(0)
        n_days, n_found, max_m = (b.to_array((K, C), np.int32) if C else np.zeros((K, 0), np.int32) for b in self.out32)
        sums = [b.to_array((K, C), np.int64) if C else np.zeros((K, 0), np.int64) for b in self.out64]
        return dict(n_days=n_days, n_found=n_found, sum_m=sums[0], sum_north_m=sums[1], sum_east_m=sums[2], max_m=max_m,
                    n_visited=int(self.count.to_array((1,), np.int64)[0]))

    def resident_bytes(self):
        return (8 * ((self.T + 63) // 64) * self.C + self.table.nbytes + 8 * self.table.ny * self.table.nx
                + 36 * self.K * self.C)

    def free(self):
        self._scope.free()


def time_blocks(T, row_bytes, budget, block_steps=None):
    """[(t0, nt)]: the time axis in blocks whose rows fit ``budget`` bytes (one step at least), or of ``block_steps``"""
    nb = int(block_steps) if block_steps else int(max(1, min(T, budget // max(row_bytes, 1))))
    if nb < 1:
        raise XmhwException("block_steps should be >= 1")
    return [(t0, min(nb, T - t0)) for t0 in range(0, T, nb)]


def _walk_time(acc, field, se_ptr, ldc, D, max_batch_bytes, block_steps):
    """The time-block walker: a block of steps of the uncompacted (T, N) host array is one contiguous range; it is
    uploaded, queued and freed, block after block, while everything else stays resident."""
    T, N = field.shape
    isz = field.dtype.itemsize
    if max_batch_bytes is None:
        max_batch_bytes = device_budget_bytes()
    budget = max(int(max_batch_bytes) - acc.resident_bytes(), 0)
    for t0, nt in time_blocks(T, N * isz, budget, block_steps):
        with DeviceScope() as s:
            d_ts = s.upload(field[t0:t0 + nt])
            acc.add_block(d_ts.ptr, isz, N, t0, nt, se_ptr, ldc, D)
            acc.h.stream_sync(0)                        # the block is freed on the way out


def displacement_grid(field, seas, rows, view, cell_index, table, classes, K, basin=None, coldSpells=False,
                      max_batch_bytes=None, block_steps=None):
    """The device stage.  ``field`` (T, ny * nx): the UNCOMPACTED host series, float32 or float64, land NaN; ``seas``
    (D, C) float64 on the C ocean cells (a host array, or a DeviceSeas); ``rows`` (T,) the climatology row of every step; ``view`` the compact_view() of
    the detection (C cells); ``cell_index`` (C,) the grid point of every ocean cell, ascending; ``table`` the
    DisplacementTable of the grid; ``classes`` (T,) int labels in [-1, K); ``basin`` None or (ny * nx,) int labels.
    Returns a dict of STAGE_FIELDS, each (K, C), plus ``n_visited``.  Time blocks below ``max_batch_bytes`` (or of
    ``block_steps`` steps) go through the device; the sums are integers, so the blocks do not change a bit."""
    if not isinstance(seas, DeviceSeas):
        seas = np.ascontiguousarray(seas, dtype=np.float64)
    field, rows, cell_of_point, classes, K, basin = check_stage_inputs(field, seas, rows, view, cell_index, table, classes,
                                                                       K, basin)
    T = field.shape[0]
    acc = _Accumulators(view, cell_of_point, table, classes, K, basin, coldSpells, T, rows)
    try:
        with DeviceScope() as s:
            if isinstance(seas, DeviceSeas):
                se_ptr, ldc = seas.ptr, seas.ld
            else:
                se_ptr, ldc = s.upload(seas).ptr, seas.shape[1]
            if acc.C:
                _walk_time(acc, np.ascontiguousarray(field), se_ptr, ldc, seas.shape[0], max_batch_bytes, block_steps)
            return acc.result()
    finally:
        acc.free()


class DisplacementDataset:
    """What mhw_displacement() returns, as plain arrays over (klass, *spatial dims).

    klass (K,) the class labels (sorted non-negative labels found), n_steps (K,) the time steps of each class;
    n_days, n_found int32, sum_m, sum_north_m, sum_east_m int64, max_m int32 (K, ...): the accumulators of the module
    docstring, in metres;
    displacement_mean_km = sum_m / (1000 * n_found), north_mean_km, east_mean_km formed the same way (NaN where
    n_found == 0); displacement_max_km = max_m / 1000 (NaN where n_found == 0); reached = n_found / n_days (NaN where
    n_days == 0).
    Land: grid lines without an ocean cell are dropped, as in ClassDaysDataset; float fields are NaN on the remaining
    land cells, integer fields are 0 there and come with the boolean ``keep`` (...) mask of the ocean cells.
    attrs: classes, max_distance_km, periodic, radius_km, n_visited, n_sources, xmhw_parameters."""

    def __init__(self, klass, n_steps, fields, keep, sdims, coords, tdim="time", attrs=None):
        self.klass, self.n_steps = np.asarray(klass), np.asarray(n_steps)
        for name in STAGE_FIELDS:
            setattr(self, name, fields[name])
        self.keep, self.sdims, self.coords = keep, tuple(sdims), dict(coords)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        found = self.n_found.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.displacement_mean_km = self.sum_m.astype(np.float64) / (1000.0 * found)
            self.north_mean_km = self.sum_north_m.astype(np.float64) / (1000.0 * found)
            self.east_mean_km = self.sum_east_m.astype(np.float64) / (1000.0 * found)
            self.displacement_max_km = self.max_m.astype(np.float64) / 1000.0
            self.reached = found / self.n_days.astype(np.float64)
        for a in (self.displacement_mean_km, self.north_mean_km, self.east_mean_km, self.displacement_max_km):
            a[self.n_found == 0] = np.nan
        self.reached[self.n_days == 0] = np.nan

    _FLOATS = ("displacement_mean_km", "north_mean_km", "east_mean_km", "displacement_max_km", "reached")

    def to_xarray(self):
        import xarray as xr
        cell = ("klass",) + self.sdims
        data = {f: (cell, getattr(self, f)) for f in STAGE_FIELDS + self._FLOATS}
        data["n_steps"] = (("klass",), self.n_steps)
        data["keep"] = (self.sdims, self.keep)
        return xr.Dataset(data, coords=dict({"klass": self.klass}, **{d: self.coords[d] for d in self.sdims if d in self.coords}),
                          attrs=self.attrs)


def _grid_axes(sdims, sshape, coords, lat, lon):
    """(latitude (ny,), nx, dlon, name of the longitude dim): the conditions of the module docstring, each refused by
    name"""
    def pick(given, names, arg, what):
        if given is not None:
            if given not in sdims:
                raise XmhwException(f"{arg}={given!r} is not a spatial dim of temp {tuple(sdims)}")
            return given
        found = [d for d in sdims if str(d).lower() in names]
        if len(found) != 1:
            raise XmhwException(f"mhw_displacement needs one {what} dim named one of {names} among {tuple(sdims)}: "
                                f"pass {arg}='name'")
        return found[0]

    if len(sdims) != 2:
        raise XmhwException(f"mhw_displacement needs two spatial dims, a latitude and a longitude, got {tuple(sdims)}")
    latd, lond = pick(lat, LAT_NAMES, "lat", "latitude"), pick(lon, LON_NAMES, "lon", "longitude")
    if latd == lond:
        raise XmhwException("lat and lon name the same dim")
    if sdims[-1] != lond:
        raise XmhwException(f"longitude ({lond!r}) should be the fast axis of the stacked layout {tuple(sdims)}: the spatial "
                            "dims are stacked in sorted-name order")
    for d in (latd, lond):
        if d not in coords or np.asarray(coords[d]).ndim != 1:
            raise XmhwException(f"dim {d!r} needs a 1-D coordinate")
    latv, lonv = np.asarray(coords[latd], dtype=np.float64), np.asarray(coords[lond], dtype=np.float64)
    ny, nx = (int(v) for v in sshape)
    if latv.shape != (ny,) or lonv.shape != (nx,):
        raise XmhwException(f"the coordinates of {latd!r} and {lond!r} do not match the grid {ny} x {nx}")
    if not np.isfinite(lonv).all():
        raise XmhwException("longitude should be finite")
    if nx > 1:
        dlon = (lonv[-1] - lonv[0]) / (nx - 1)
        if dlon == 0.0 or np.abs(np.diff(lonv) - dlon).max() > 1e-6 * abs(dlon):
            raise XmhwException(f"longitude should be uniformly spaced: the spacings differ from dlon={dlon} by more than "
                                "1e-6, relative")
    else:
        dlon = 0.0
    return latv, nx, float(dlon), lond


def mhw_displacement(temp, th, se, mhw, classes="all", max_distance=1000.0, periodic=None, basin=None,
                     radius=EARTH_RADIUS_KM, lat=None, lon=None, tdim="time", maxPadLength=None, coldSpells=False,
                     tstep=False, anynans=False, _compute=None, max_batch_bytes=None):
    """The thermal displacement of every MHW cell-day, per cell and class of time steps.

    ``temp``, ``th``, ``se`` and the options shared with detect() mean and validate what they do there and in
    mhw_days_by() (same exceptions, land masking and positional pairing of series and climatology cells); give what
    detect() was given, and ``mhw``, the EventDataset it returned.  ``classes``: as in mhw_days_by().  ``max_distance``
    (km): how far a source looks.  ``periodic``: None, or the name of the longitude dim when the grid wraps there.
    ``basin``: None, or one integer label per grid point (any shape of ny * nx entries): a destination has to carry the
    source's label; a source with a negative label is skipped.  ``radius`` in km.  ``lat``, ``lon``: the names of the
    latitude and longitude dims when they are not lat / latitude and lon / longitude.  ``maxPadLength`` is refused:
    destination samples are read as stored.

    Returns a DisplacementDataset (module docstring: the definition; class docstring: the fields).  Every result is an
    exact integer, the same from run to run and for every ``max_batch_bytes``.  ``_compute``: a stand-in for
    displacement_grid() (host tests)."""
    from .detect import EventDataset
    from .detect_front import _check_inputs
    if not isinstance(mhw, EventDataset):
        raise XmhwException("mhw_displacement expects the EventDataset returned by xmhw_amd.detect()")
    if maxPadLength is not None:
        raise XmhwException("mhw_displacement does not take maxPadLength: destination samples are read as stored")
    layout = grid_layout(temp, tdim)
    coords, _, dims, point, sdims, sshape, N = layout
    if point or mhw.point:
        raise XmhwException("mhw_displacement needs a grid: a single-point series has no neighbours")
    latv, nx, dlon, lond = _grid_axes(sdims, sshape, coords, lat, lon)
    params = mhw.attrs.get("xmhw_parameters")
    if params is not None and (_COLD_TEXT in params) != bool(coldSpells):
        raise XmhwException(f"coldSpells={bool(coldSpells)} differs from the detection's recorded parameters")
    sshape = tuple(int(v) for v in sshape)
    if tuple(mhw.sdims) != tuple(sdims) or tuple(int(v) for v in mhw.sshape) != sshape:
        raise XmhwException(f"temp is on the grid {dict(zip(sdims, sshape))}, the detection on "
                            f"{dict(zip(mhw.sdims, mhw.sshape))}: mhw does not belong to temp")
    time = np.asarray(coords[tdim])
    T = int(time.shape[0])
    if np.asarray(mhw.time).shape[0] != T:
        raise XmhwException(f"temp has {T} time steps, the detection {np.asarray(mhw.time).shape[0]}")
    if is_packed(temp.values):
        raise XmhwException("mhw_displacement does not read packed int16 views: pass decoded floats")
    if periodic is not None and periodic != lond:
        raise XmhwException(f"periodic should be None or the name of the longitude dim ({lond!r}), got {periodic!r}")
    basin = _check_basin(basin, N)
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "mhw_displacement", "classes")
    n_steps = np.bincount(kid[kid >= 0], minlength=K).astype(np.int64)
    budget = device_budget_bytes() if max_batch_bytes is None else int(max_batch_bytes)
    table = displacement_offsets(latv, nx, dlon, max_distance, periodic is not None, radius, max_table_bytes=budget // 4)
    view = mhw.compact_view()
    keep_want = np.asarray(mhw.keep, dtype=bool).reshape(-1)
    cell_index = view["cell_index"]
    got = {}

    def on_cells(host_keep, ts, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells_, **extra):
        # _detect() has masked and compacted on the host (a stand-in stage): the stage still reads the field as stored
        from .landmask import stack_cells
        if not np.array_equal(host_keep(), keep_want):
            raise XmhwException("the land mask of temp differs from mhw.keep: mhw does not belong to temp")
        _, sec, _, rows = _check_inputs(ts, sec, thc, doy, doys)
        field = stack_cells(np.asarray(temp.values), dims, tdim)[0]
        got["stage"] = _compute(field, sec, rows, view, cell_index, table, kid, K, basin=basin, coldSpells=coldSpells_)

    def on_grid(stacked, anynans_, sec, thc, doy, doys, minDuration, joinGaps, maxGap, coldSpells_, max_batch_bytes=None,
                clim_stacked=False, pad=None):
        from .detect_front import _rows_as_they_are
        if is_packed(stacked):
            raise XmhwException("mhw_displacement does not read packed int16 views: pass decoded floats")
        if stacked.shape[1] != keep_want.shape[0]:
            raise XmhwException(f"temp has {stacked.shape[1]} grid points, the detection {keep_want.shape[0]}: mhw does not "
                                "belong to temp")
        sec, thc = _rows_as_they_are(sec), _rows_as_they_are(thc)
        if sec.ndim != 2 or thc.ndim != 2 or sec.shape[0] != thc.shape[0]:
            raise XmhwException("seas and thresh must be (D, cells) arrays")
        sample = np.zeros((stacked.shape[0], 1), dtype=native_float(stacked[:1, :1]).dtype)
        rows = _check_inputs(sample, sec[:, :1], thc[:, :1], doy, doys)[3]
        with DeviceScope() as clim:
            d_se, _, C = climatologies_on_device(clim, sec, thc, anynans_, clim_stacked)
            if C != view["C"]:
                raise XmhwException(f"th and se have {C} ocean cells, the detection {view['C']}: mhw does not belong to temp")
            got["stage"] = displacement_grid(stacked, DeviceSeas(d_se.ptr, C, sec.shape[0], C), rows, view, cell_index, table,
                                             kid, K, basin=basin, coldSpells=coldSpells_, max_batch_bytes=max_batch_bytes)
        if not keep_want.any():
            raise XmhwException(LAND_TEXT)
        return keep_want

    res = run(temp, th, se, layout, tdim, on_cells, on_grid, None, coldSpells, tstep, anynans, _compute, max_batch_bytes)
    st = got["stage"]
    f = CellFrame(res.keep, res.cell_index, False, sdims, sshape, coords)
    C = f.C
    fields = {}
    for name, dtype in _STAGE.items():
        a = np.asarray(st[name])
        if a.shape != (K, C):
            raise XmhwException(f"displacement stage returned {name} of shape {a.shape}, expected {(K, C)}")
        fields[name] = a.astype(dtype)
    klass = found if found.shape[0] else np.zeros(1, dtype=np.int64)
    attrs = {"classes": classes if isinstance(classes, str) else "array", "max_distance_km": float(max_distance),
             "periodic": periodic, "radius_km": float(radius), "n_visited": int(st["n_visited"]),
             "n_sources": int(fields["n_days"].sum()), "xmhw_parameters": res.attrs["xmhw_parameters"]}
    return DisplacementDataset(klass, n_steps, {n: f.place(fields[n], 0, d) for n, d in _STAGE.items()}, f.keep, f.sdims,
                               f.coords, tdim, attrs)
