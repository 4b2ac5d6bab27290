"""spatial_correlation(): per-cell correlation with grid neighbours -- the spatial correlation function of the anomaly
and its decorrelation length: how large heatwaves are, the spatial counterpart of the e-folding time of
lag_correlation(), and the input to every field-significance statement (the effective number of independent cells of a
map comes from it).  Every other stage reduces over time and keeps the cell; this one relates the series of a cell to
the series of the cells around it.  One pass over the resident, UNCOMPACTED grid in time blocks
(csrc/kernels_spatialcorr.hip, csrc/halo_tile.h).

The definition (include/xmhw_amd.h, "spatial_correlation()", states it for the C entries).  Inputs: the uncompacted series
ts[T][ny * nx] (float32 or float64, land NaN, longitude the fast axis), a base[Dr][ny * nx] float64 on the same grid with
row_of_t[T] (one row: a constant per point), a shift in [0, 24], labels class_of_t[T] in [-1, K), K <= 64, ``periodic``
(longitude wraps), T < 2**17, ny, nx <= 32767, and D offsets (dj, di), 1 <= D <= 64, |dj|, |di| <= 32; duplicates and
(0, 0) are allowed; on a periodic grid |di| < nx.
    a(t, p) = (float64(ts[t, p]) - base[row_of_t[t], p]) * 2**-shift                   (the scaling is exact)
    a sample is VALID iff a is not NaN and |a| < 2**7; q = rint(a * 2**16).
For every grid point p = (j, i), every step t with k = class_of_t[t] >= 0 and every offset e = (dj, di) the partner is
p' = (j + dj, i + di), i + di taken mod nx when periodic; the pair is valid iff p' lies in the grid and a(t, p) and
a(t, p') are both valid, and a valid pair adds
    n[k, e, p] += 1 (int32);  sx += q(p), sy += q(p'), sxx += q(p)**2, syy += q(p')**2, sxy += q(p) q(p')   (int64).
Pairwise deletion, as in lag_correlation().  Land points keep n = 0; steps of class -1 are not read.  n_range counts the
(t, p) of class >= 0 whose a is not NaN and out of range, each once; such a sample is no partner either.  |q| <= 2**23,
products <= 2**46, fewer than 2**17 pairs per entry: everything stays inside 64 bits.  Everything is an integer sum: the
result does not depend on the time blocks, the tile geometry, the offset grouping or the schedule.

The device computes (0, 0) and the HALF-PLANE of the request (dj > 0, or dj == 0 and di > 0); the mirrored offsets are
filled on the host from the identity: the sums of -e at p are those of +e at p - e with x and y exchanged (across a
periodic seam the shift wraps; a partner off the grid gives n = 0).  The identity is exact.

Host side here (offsets, the half-plane, the base on the grid, time blocks, derived fields); device side behind
spatial_corr_grid().
"""
import math

import numpy as np

from ._lib import hip_spatialcorr
from .device import DeviceScope, as_xmhw_errors, device_budget_bytes, is_packed, native_float
from .displacement import EARTH_RADIUS_KM, _grid_axes, pair_metrics, time_blocks
from .exception import XmhwException
from .series_stage import (Accumulators, check_class_ids, check_steps, class_labels, class_result_labels, dense_ids,
                           grid_layout, ocean_mask, report_range)

MAX_OFFSETS = 64                # XMHW_SPATIAL_CORR_MAX_OFFSETS (include/xmhw_amd.h)
REACH = 32                      # XMHW_SPATIAL_CORR_REACH
MAX_CLASSES = 64                # XMHW_SPATIAL_CORR_MAX_CLASSES
MAX_AXIS = 32767                # XMHW_SPATIAL_CORR_MAX_AXIS
BITS = 16                       # XMHW_SPATIAL_CORR_BITS
RANGE_BITS = 7                  # |a| < 2**7
MAX_SHIFT = 24                  # XMHW_SPATIAL_CORR_MAX_SHIFT
FIELDS = ("n", "sx", "sy", "sxx", "syy", "sxy")
_SWAPPED = ("n", "sy", "sx", "syy", "sxx", "sxy")       # the same sums with the roles of the two points exchanged
BYTES_PER_ENTRY = 44            # int32 n and five int64 sums
CROSS_STEPS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
AXES = ("zonal", "meridional")


def _range_texts(shift):
    """the refusal of out-of-range samples, by the key of the counter (the pattern of lag_correlation._range_texts)"""
    return {"n_range": (f"samples of x lie 2**(7 + shift) and more from their base (or are infinite) with shift = {shift}: "
                        "pass a larger shift (heat flux in W m-2 needs a shift of 4 or so)")}


# ---- validation (mirrors the refusals of the C entries) ----------------------------------------------

def check_shift(shift):
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)):
        raise XmhwException(f"shift should be a whole number, got {shift!r}")
    if not 0 <= int(shift) <= MAX_SHIFT:
        raise XmhwException(f"shift should be in [0, {MAX_SHIFT}], got {int(shift)}")
    return int(shift)


def check_offsets(offsets, nx=None, periodic=False):
    """(D, 2) int32 offsets (dj, di) as the C entries take them: 1 <= D <= 64 whole numbers within the reach of 32 points;
    on a periodic grid of nx columns |di| < nx"""
    try:
        a = np.asarray(offsets)
    except (TypeError, ValueError):
        a = None
    if a is None or a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in "iu":
        raise XmhwException(f"offsets should be a sequence of (dj, di) pairs of whole numbers of grid points, got {offsets!r}")
    if not 1 <= a.shape[0] <= MAX_OFFSETS:
        raise XmhwException(f"spatial_correlation handles 1 to {MAX_OFFSETS} offsets a pass, got {a.shape[0]}")
    if np.abs(a.astype(np.int64)).max() > REACH:
        raise XmhwException(f"spatial_correlation reaches at most {REACH} grid points either way, got offsets up to "
                            f"{int(np.abs(a.astype(np.int64)).max())}: coarsen the grid first")
    if periodic and nx is not None and np.abs(a[:, 1].astype(np.int64)).max() >= nx:
        raise XmhwException(f"on a periodic grid of {nx} columns an offset should have |di| < {nx}")
    return np.ascontiguousarray(a, dtype=np.int32)


def cross_offsets(reach):
    """The cross of ``reach`` = (ry, rx): (0, 0) and the steps 1, 2, 3, 4, 6, 8, 12, 16, 24, 32 up to the reach either way
    on each axis, as (D, 2) int32 in ascending (dj, di) order"""
    try:
        ry, rx = reach
    except (TypeError, ValueError):
        raise XmhwException(f"reach should be a pair (ry, rx) of whole numbers of grid points, got {reach!r}") from None
    for v in (ry, rx):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise XmhwException(f"reach should be a pair (ry, rx) of whole numbers of grid points, got {reach!r}")
        if not 0 <= int(v) <= REACH:
            raise XmhwException(f"reach should be in [0, {REACH}] on each axis, got {reach!r}: coarsen the grid first")
    out = {(0, 0)}
    for s in CROSS_STEPS:
        if s <= int(ry):
            out.update({(s, 0), (-s, 0)})
        if s <= int(rx):
            out.update({(0, s), (0, -s)})
    return np.array(sorted(out), dtype=np.int32)


def check_result_bytes(K, D, N, max_result_bytes):
    """the (K, D, ny * nx) accumulators, 44 bytes an entry, live on the device across the blocks and come back whole"""
    need = BYTES_PER_ENTRY * K * D * N
    if max_result_bytes is not None and need > max_result_bytes:
        raise XmhwException(f"the sums of K = {K} classes x {D} offsets x {N} grid points take {need} bytes, more than "
                            f"max_result_bytes = {int(max_result_bytes)}: use fewer classes, fewer offsets or a part of "
                            "the grid")


# ---- the half-plane and its mirror ---------------------------------------------------------------------

def half_plane(offsets):
    """(device offsets (Dh, 2) int32, index (D,), mirrored (D,) bool): (0, 0) first, then the distinct offsets of the
    request folded into the half-plane dj > 0, or dj == 0 and di > 0, ascending; request entry e is device entry index[e],
    mirrored[e] where the request holds its negative"""
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 2)
    neg = (offsets[:, 0] < 0) | ((offsets[:, 0] == 0) & (offsets[:, 1] < 0))
    folded = np.where(neg[:, None], -offsets, offsets)
    rest = sorted({(int(a), int(b)) for a, b in folded} - {(0, 0)})
    dev = [(0, 0)] + rest
    where = {e: i for i, e in enumerate(dev)}
    index = np.array([where[(int(a), int(b))] for a, b in folded], dtype=np.int64)
    return np.array(dev, dtype=np.int32).reshape(-1, 2), index, neg


def shift_back(a, dj, di, periodic):
    """b[..., j, i] = a[..., j - dj, i - di], zero where (j - dj, i - di) leaves the grid; across a periodic seam the
    column wraps"""
    ny, nx = a.shape[-2:]
    out = np.zeros_like(a)
    if abs(dj) >= ny:
        return out
    dst_j, src_j = slice(max(0, dj), min(ny, ny + dj)), slice(max(0, -dj), min(ny, ny - dj))
    if periodic:
        out[..., dst_j, :] = np.roll(a[..., src_j, :], di, axis=-1)
    elif abs(di) < nx:
        dst_i, src_i = slice(max(0, di), min(nx, nx + di)), slice(max(0, -di), min(nx, nx - di))
        out[..., dst_j, dst_i] = a[..., src_j, src_i]
    return out


def mirror_fill(sums, dev_offsets, index, mirrored, ny, nx, periodic):
    """The six arrays (K, D, ny, nx) of the request from those of the device pass (K, Dh, ny * nx): an entry of the
    half-plane as it is; its negative -e at p from +e at p - e with x and y exchanged"""
    sums = dict(zip(FIELDS, (np.asarray(a).reshape(a.shape[0], a.shape[1], ny, nx) for a in sums)))
    out = []
    for name, other in zip(FIELDS, _SWAPPED):
        parts = []
        for e, m in zip(index, mirrored):
            if m:
                dj, di = (int(v) for v in dev_offsets[e])
                parts.append(shift_back(sums[other][:, e], dj, di, periodic))
            else:
                parts.append(sums[name][:, e])
        out.append(np.stack(parts, axis=1))
    return tuple(out)


# ---- the device stage --------------------------------------------------------------------------------

class _Accumulators(Accumulators):
    """One call's device accumulators (FIELDS, (K, D, ny * nx)) with the range counter and the resident base; add_block()
    ADDS a block of steps, one after the other on the stream without a read-back."""

    def __init__(self, base, rows, classes, K, offsets, ny, nx, periodic, shift, T):
        super().__init__()
        self.hs = hip_spatialcorr()
        self.ny, self.nx, self.periodic, self.shift, self.T = int(ny), int(nx), int(bool(periodic)), int(shift), int(T)
        self.N = self.ny * self.nx
        self.classes, self.K, self.offsets, self.rows = classes, int(K), offsets, rows
        self.range_texts = _range_texts(self.shift)
        D = offsets.shape[0]
        try:
            self.make(self.N, {k: ((self.K, D, self.N), np.int32 if k == "n" else np.int64) for k in FIELDS})
            self.Dr = int(base.shape[0])
            self.base = self._scope.upload(base)
            with as_xmhw_errors(also="Unsupported"):
                self.hs.spatial_corr_init(self.K, D, self.ny, self.nx, *self.ptrs(), self.N, self.count.ptr)
        except BaseException:
            self.free()
            raise

    def resident_bytes(self):
        return BYTES_PER_ENTRY * self.K * self.offsets.shape[0] * self.N + 8 * self.Dr * self.N

    def add_block(self, ts_ptr, isz, ld, t0, nt):
        """the steps t0 .. t0 + nt - 1: their uncompacted rows are at ts_ptr, leading dimension ld >= ny * nx"""
        with as_xmhw_errors(also="Unsupported"):
            self.hs.spatial_corr_accumulate(ts_ptr, isz, ld, t0, nt, self.T, self.ny, self.nx, self.periodic, self.base.ptr,
                                            self.N, self.Dr, self.rows, self.shift, self.classes, self.K, self.offsets,
                                            *self.ptrs(), self.N, self.count.ptr)


def _walk_time(acc, field, max_batch_bytes, block_steps):
    """The time-block walker of displacement._walk_time: a block of steps of the uncompacted (T, N) host array is one
    contiguous range; it is uploaded, queued and freed, block after block, while everything else stays resident."""
    T, N = field.shape
    isz = field.dtype.itemsize
    if max_batch_bytes is None:
        max_batch_bytes = device_budget_bytes()
    budget = max(int(max_batch_bytes) - acc.resident_bytes(), 0)
    for t0, nt in time_blocks(T, N * isz, budget, block_steps):
        with DeviceScope() as s:
            d_ts = s.upload(field[t0:t0 + nt])
            acc.add_block(d_ts.ptr, isz, N, t0, nt)
            acc.h.stream_sync(0)                        # the block is freed on the way out


def check_stage_inputs(field, base, rows, classes, K, offsets, ny, nx, periodic, shift):
    """What both stages (the device's and a stand-in) may rely on: (field, base, rows, classes, K, offsets, shift) checked
    and in the layouts the device takes"""
    if is_packed(field):
        raise XmhwException("spatial_correlation does not read packed int16 views: pass decoded floats")
    field = np.ascontiguousarray(native_float(np.asarray(field)))
    ny, nx = int(ny), int(nx)
    if ny < 1 or nx < 1 or ny > MAX_AXIS or nx > MAX_AXIS:
        raise XmhwException(f"spatial_correlation handles grid axes of 1 to {MAX_AXIS} points, got {ny} x {nx}")
    N = ny * nx
    if field.ndim != 2 or field.shape[1] != N:
        raise XmhwException(f"the series should be (T, {N}) on the {ny} x {nx} grid, got {field.shape}")
    T = field.shape[0]
    if T < 1:
        raise XmhwException("the series has no time step")
    check_steps(T, "spatial_correlation")
    base = np.ascontiguousarray(base, dtype=np.float64)
    if base.ndim != 2 or base.shape[1] != N or base.shape[0] < 1:
        raise XmhwException(f"the base should be (Dr, {N}) on the grid of the series, got {base.shape}")
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.shape != (T,) or rows.min() < 0 or rows.max() >= base.shape[0]:
        raise XmhwException("rows should hold the base row of every time step")
    classes, K = check_class_ids(T, classes, K, MAX_CLASSES, "spatial_correlation")
    return field, base, rows, classes, K, check_offsets(offsets, nx, periodic), check_shift(shift)


def spatial_corr_grid(field, base, rows, classes, K, offsets, ny, nx, periodic=False, shift=0, max_batch_bytes=None,
                      block_steps=None, counters=None, max_result_bytes=None):
    """The device stage.  ``field`` (T, ny * nx): the UNCOMPACTED host series, float32 or float64, land NaN; ``base``
    (Dr, ny * nx) float64 with ``rows`` (T,) the base row of every step; ``classes`` (T,) int labels in [-1, K);
    ``offsets`` (D, 2) the (dj, di) of the definition, as they are (no half-plane here).  Returns the six arrays of
    FIELDS, each (K, D, ny * nx).  Time blocks below ``max_batch_bytes`` (or of ``block_steps`` steps) go through the
    device; the sums are integers, so the blocks do not change a bit.  Raises if a sample is out of range (module
    docstring); with ``counters`` (a dict) it stores ``n_range`` there instead."""
    field, base, rows, classes, K, offsets, shift = check_stage_inputs(field, base, rows, classes, K, offsets, ny, nx,
                                                                       periodic, shift)
    check_result_bytes(K, offsets.shape[0], int(ny) * int(nx), max_result_bytes)
    acc = _Accumulators(base, rows, classes, K, offsets, ny, nx, periodic, shift, field.shape[0])
    try:
        _walk_time(acc, field, max_batch_bytes, block_steps)
        out, n_range = acc.result()
    finally:
        acc.free()
    report_range(n_range, counters, acc.range_texts)
    return out


# ---- the result --------------------------------------------------------------------------------------

def _first_below(r, level):
    """(index of the first entry below ``level`` along axis 0 past entry 0, whether there is one)"""
    below = r < level
    below[0] = False
    return below.argmax(axis=0), below.any(axis=0)


def _pair_mean(a, b):
    """the mean of two arrays where both are numbers, the one that is where the other is NaN"""
    both = ~np.isnan(a) & ~np.isnan(b)
    return np.where(both, 0.5 * (a + b), np.where(np.isnan(a), b, a))


class SpatialCorrelationDataset:
    """What spatial_correlation() returns, as plain arrays over (klass, offset, lat, lon) on the whole grid (no grid line
    is dropped: the neighbours of a cell are grid neighbours).

    klass (K,) the class labels (sorted non-negative labels found), offset (D, 2) the (dj, di) of the request, shift,
    periodic, lat (ny,) degrees, dlon degrees, radius km.
    Raw integers: n int32 and sx, sy, sxx, syy, sxy int64 (module docstring), x the cell itself and y its partner, in
    units of 2**(shift - 16).
    Derived float64, one fixed formula on the integers as in LagCorrelationDataset, from mx = sx / n, my = sy / n:
        mean_x   mx * 2**(shift - 16), mean_y likewise: the means over the PAIRS of the offset, in original units
        cov      (sxy / n - mx my) * 2**(2 shift - 32)
        r        (sxy / n - mx my) / sqrt((sxx / n - mx**2) (syy / n - my**2)): Pearson's correlation of the pairs
        slope    (sxy / n - mx my) / (syy / n - my**2): the cell per unit of its partner
    all NaN where n < 2 (land, a partner off the grid); r and slope NaN where a variance is zero as well.
    keep (ny, nx): the ocean cells of x."""

    def __init__(self, klass, offset, n, sx, sy, sxx, syy, sxy, keep, sdims, coords, lat, dlon, shift=0, periodic=False,
                 radius=EARTH_RADIUS_KM, tdim="time", attrs=None):
        self.klass, self.offset = np.asarray(klass), np.asarray(offset, dtype=np.int32).reshape(-1, 2)
        self.n, self.sx, self.sy, self.sxx, self.syy, self.sxy = n, sx, sy, sxx, syy, sxy
        self.keep, self.sdims, self.coords = np.asarray(keep, dtype=bool), tuple(sdims), dict(coords)
        self.lat, self.dlon, self.radius = np.asarray(lat, dtype=np.float64), float(dlon), float(radius)
        self.shift, self.periodic = int(shift), bool(periodic)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        nf = n.astype(np.float64)
        f = lambda a: a.astype(np.float64)                                                           # noqa: E731
        few = n < 2
        with np.errstate(divide="ignore", invalid="ignore"):
            mx, my = f(sx) / nf, f(sy) / nf
            cov, vx, vy = f(sxy) / nf - mx * my, f(sxx) / nf - mx * mx, f(syy) / nf - my * my
            flat = few | ~(vx > 0.0) | ~(vy > 0.0) | self._no_spread(n, sx, sxx, vx) | self._no_spread(n, sy, syy, vy)
            unit = 2.0 ** (self.shift - BITS)
            self.mean_x = np.where(few, np.nan, mx * unit)
            self.mean_y = np.where(few, np.nan, my * unit)
            self.cov = np.where(few, np.nan, cov * unit * unit)
            self.r = np.where(flat, np.nan, cov / np.sqrt(vx * vy))
            self.slope = np.where(flat, np.nan, cov / vy)
        self._vx, self._vy, self._cov_q = np.where(flat, np.nan, vx), np.where(flat, np.nan, vy), np.where(flat, np.nan, cov)

    @staticmethod
    def _no_spread(n, s, ss, v):
        # a variance is zero iff n ss == s**2: the product wraps in 64 bits, so that is asked of a variance that float64
        # finds negligible as well (LagCorrelationDataset._no_spread)
        with np.errstate(over="ignore"):
            wraps = n.astype(np.uint64) * ss.astype(np.uint64) == s.astype(np.uint64) * s.astype(np.uint64)
        return wraps & (np.abs(v) <= 2.0 ** -40 * (ss.astype(np.float64) / np.maximum(n, 1)))

    def _at(self, dj, di):
        i = np.nonzero((self.offset[:, 0] == dj) & (self.offset[:, 1] == di))[0]
        return int(i[0]) if i.size else None

    def distance_km(self):
        """(D, ny) float64: the great-circle distance in km from a cell of latitude row j to its partner at every offset
        (displacement.pair_metrics, metres rounded to whole numbers), NaN where the partner's row is off the grid"""
        ny = self.lat.shape[0]
        phi = np.deg2rad(self.lat)
        j = np.arange(ny)
        out = np.full((self.offset.shape[0], ny), np.nan)
        for e, (dj, di) in enumerate(self.offset):
            ok = (j + dj >= 0) & (j + dj < ny)
            dist = pair_metrics(phi[ok], phi[j[ok] + dj], math.radians(float(di) * self.dlon), self.radius)[0]
            out[e, ok] = dist / 1000.0
        return out

    def efolding_length(self, axis):
        """The e-folding (decorrelation) length in km along ``axis``, "zonal" (offsets (0, +-s)) or "meridional"
        ((+-s, 0)), over (klass, lat, lon): with s the steps of the request on that axis, ascending, r(s) the mean of r at
        +s and -s (the one that is a number where the other is not: at an edge) and d(s) the mean of their distances
        likewise, r(0) = 1 at distance 0 on the ocean cells: the first s at which r(s) < 1 / e, linearly interpolated in
        distance between it and the step before -- the crossing rule of LagCorrelationDataset.efolding_time().  NaN where
        1 / e is not reached within the request, where the step before the crossing has no correlation, and on land."""
        if axis not in AXES:
            raise XmhwException(f"axis should be one of {AXES}, got {axis!r}")
        zonal = axis == "zonal"
        along, across = (1, 0) if zonal else (0, 1)
        on = self.offset[self.offset[:, across] == 0]
        steps = sorted({abs(int(v)) for v in on[:, along]} - {0})
        if not steps:
            raise XmhwException(f"the request holds no {axis} offset")
        dist = self.distance_km()
        K, _, ny, nx = self.r.shape
        r = np.full((len(steps) + 1, K, ny, nx), np.nan)
        d = np.zeros((len(steps) + 1, ny))
        r[0] = np.where(self.keep, 1.0, np.nan)
        for m, s in enumerate(steps, start=1):
            both = [self._at(*((0, v) if zonal else (v, 0))) for v in (s, -s)]
            rs = [self.r[:, e] for e in both if e is not None]
            ds = [dist[e] for e in both if e is not None]
            r[m] = rs[0] if len(rs) == 1 else _pair_mean(rs[0], rs[1])
            d[m] = ds[0] if len(ds) == 1 else _pair_mean(ds[0], ds[1])
        level = math.exp(-1.0)
        i, some = _first_below(r, level)
        i1 = np.maximum(i, 1)
        hi_ = np.take_along_axis(r, (i1 - 1)[None], axis=0)[0]
        lo_ = np.take_along_axis(r, i1[None], axis=0)[0]
        dd = np.broadcast_to(d[:, None, :, None], r.shape)
        d_hi = np.take_along_axis(dd, (i1 - 1)[None], axis=0)[0]
        d_lo = np.take_along_axis(dd, i1[None], axis=0)[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            out = d_hi + (hi_ - level) / (hi_ - lo_) * (d_lo - d_hi)
        return np.where(some, out, np.nan)

    def anisotropy(self):
        """efolding_length("zonal") / efolding_length("meridional"), NaN where either is"""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.efolding_length("zonal") / self.efolding_length("meridional")

    def quantisation_bound(self):
        """What the fixed point costs r, as a dict: ``unit`` h = 2**(shift - 17), the half unit by which a sample is off,
        and ``r``, a bound on |r - the correlation of the unquantised anomalies| like ``r``.  With h = 1 / 2 in units of
        q, sx, sy the standard deviations and c the covariance of the quantised pairs: an error in [-h, h] has a standard
        deviation of at most h, so the covariance moves by at most Dc = h (sx + sy) + h**2 and a variance by at most
        Dv = 2 h s + h**2; with Lx = sx**2 - Dvx, Ly likewise, the bound is Dc / sqrt(Lx Ly) + |c| (1 / sqrt(Lx Ly) -
        1 / (sx sy)); infinite where Lx <= 0 or Ly <= 0: the spread of the cell is not above the resolution."""
        h = 0.5
        with np.errstate(divide="ignore", invalid="ignore"):
            sx, sy = np.sqrt(self._vx), np.sqrt(self._vy)
            dc = h * (sx + sy) + h * h
            lx, ly = self._vx - (2 * h * sx + h * h), self._vy - (2 * h * sy + h * h)
            ok = (lx > 0.0) & (ly > 0.0)
            root = np.sqrt(np.where(ok, lx * ly, np.nan))
            bound = np.where(ok, dc / root + np.abs(self._cov_q) * (1.0 / root - 1.0 / (sx * sy)), np.inf)
        return {"unit": 2.0 ** (self.shift - BITS - 1), "r": np.where(np.isnan(self._vx), np.nan, bound)}

    def to_xarray(self):
        import xarray as xr
        cell = ("klass", "offset") + self.sdims
        data = {k: (cell, getattr(self, k)) for k in FIELDS + ("mean_x", "mean_y", "cov", "r", "slope")}
        data.update(keep=(self.sdims, self.keep), dj=(("offset",), self.offset[:, 0]), di=(("offset",), self.offset[:, 1]),
                    distance_km=(("offset", self.sdims[0]), self.distance_km()))
        return xr.Dataset(data, coords=dict({"klass": self.klass}, **{d: self.coords[d] for d in self.sdims if d in self.coords}),
                          attrs=dict(self.attrs, shift=self.shift, periodic=int(self.periodic)))


# ---- the public function -----------------------------------------------------------------------------

def _base_on_grid(base, ocean, sdims, sshape, coords, time):
    """(base (Dr, N) float64 with NaN on the land of x and zero where the base itself is missing on an ocean cell, rows
    (T,) int32): None is zero; a constant per cell is one row; a ('doy', ...) climatology pairs with the steps by their
    day-of-year label, as th / se do in detect()"""
    from . import calendar as cal
    from .detect_front import _check_inputs
    from .lag_correlation import _base_on_ocean
    b = _base_on_ocean(base, ocean, False, sdims, sshape, coords, "base")
    v = np.asarray(b.values, dtype=np.float64)
    v = np.transpose(v, [b.dims.index("doy")] + [b.dims.index(d) for d in sdims]).reshape(v.shape[b.dims.index("doy")], -1)
    T = np.asarray(time).shape[0]
    if v.shape[0] == 1:
        return np.ascontiguousarray(v), np.zeros(T, dtype=np.int32)
    doy = cal.add_doy(np.asarray(time))
    rows = _check_inputs(np.zeros((T, 1)), v[:, :1], v[:, :1], doy, np.asarray(b.coords["doy"]))[3]
    return np.ascontiguousarray(v), rows


def spatial_correlation(x, base=None, offsets=None, reach=None, classes="all", shift=0, periodic=None, lat=None, lon=None,
                        tdim="time", anynans=False, max_batch_bytes=None, max_result_bytes=8 << 30, block_steps=None,
                        _compute=None):
    """Correlation of every cell with its grid neighbours: for every class of time steps and every offset (dj, di), the
    sums behind the correlation of ``x - base`` at a cell with ``x - base`` at the cell dj rows and di columns away, at the
    same step.

    ``x``, ``base`` and ``classes`` are taken as lag_correlation() takes ``x``, ``base_x`` and ``classes``: a constant
    base per cell or a ('doy', ...) climatology on the grid of ``x``, None = zero; at most 64 classes.  ``x`` is a grid
    with one latitude and one longitude dim (``lat``, ``lon``: their names when they are not lat / latitude and lon /
    longitude), longitude the fast axis of the stacked layout and uniformly spaced, as in mhw_displacement();
    ``periodic``: None, or the name of the longitude dim when the grid wraps there.  Samples are read as stored.
    ``offsets``: a sequence of (dj, di), at most 32 points either way; or ``reach`` = (ry, rx): the cross of (0, 0) and the
    steps 1, 2, 3, 4, 6, 8, 12, 16, 24, 32 up to the reach either way on each axis; neither: reach=(8, 8).  The device
    computes (0, 0) and the half-plane of the request, at most 64 offsets; the mirrored half is filled on the host.
    ``shift``: samples enter as (x - base) * 2**-shift and must then lie inside (-2**7, 2**7).  The (klass, offset, grid)
    accumulators take 44 bytes an entry: the call raises before any allocation if that exceeds ``max_result_bytes``.
    ``block_steps``: the steps of a time block on the device (None: what fits ``max_batch_bytes``).

    Returns a SpatialCorrelationDataset.  Raises if a sample is out of range.  ``_compute``: a stand-in for
    spatial_corr_grid() (host tests)."""
    from .landmask import stack_cells
    if offsets is not None and reach is not None:
        raise XmhwException("pass offsets or reach, not both")
    request = check_offsets(offsets) if offsets is not None else cross_offsets((8, 8) if reach is None else reach)
    shift = check_shift(shift)
    coords, _, dims, point, sdims, sshape, N = grid_layout(x, tdim)
    if point:
        raise XmhwException("spatial_correlation needs a grid: a single-point series has no neighbours")
    latv, nx, dlon, lond = _grid_axes(sdims, sshape, coords, lat, lon)
    ny = int(latv.shape[0])
    if ny > MAX_AXIS or nx > MAX_AXIS:
        raise XmhwException(f"spatial_correlation handles grid axes of at most {MAX_AXIS} points, got {ny} x {nx}")
    if periodic is not None and periodic != lond:
        raise XmhwException(f"periodic should be None or the name of the longitude dim ({lond!r}), got {periodic!r}")
    wraps = periodic is not None
    check_offsets(request, nx, wraps)
    if is_packed(x.values):
        raise XmhwException("spatial_correlation does not read packed int16 views: pass decoded floats")
    time = np.asarray(coords[tdim])
    T = int(time.shape[0])
    check_steps(T, "spatial_correlation")
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "spatial_correlation", "classes")
    dev_offsets, index, mirrored = half_plane(request)
    if dev_offsets.shape[0] > MAX_OFFSETS:
        raise XmhwException(f"the half-plane of the request holds {dev_offsets.shape[0]} offsets with (0, 0), more than "
                            f"{MAX_OFFSETS}")
    check_result_bytes(K, dev_offsets.shape[0], N, max_result_bytes)
    ocean = ocean_mask(x, dims, tdim, False, anynans)
    base_rows, rows = _base_on_grid(base, ocean, sdims, tuple(int(v) for v in sshape), coords, time)
    field = stack_cells(np.asarray(x.values), dims, tdim)[0]
    if _compute is not None:
        sums = _compute(field, base_rows, rows, kid, K, dev_offsets, ny, nx, periodic=wraps, shift=shift)
    else:
        sums = spatial_corr_grid(field, base_rows, rows, kid, K, dev_offsets, ny, nx, periodic=wraps, shift=shift,
                                 max_batch_bytes=max_batch_bytes, block_steps=block_steps)
    want = (K, dev_offsets.shape[0], N)
    sums = [np.asarray(a) for a in sums]
    if len(sums) != 6 or any(a.shape != want for a in sums):
        raise XmhwException(f"spatial correlation stage returned {[a.shape for a in sums]}, expected six of {want}")
    raw = mirror_fill(sums, dev_offsets, index, mirrored, ny, nx, wraps)
    raw = [np.ascontiguousarray(a, dtype=np.int32 if k == "n" else np.int64) for k, a in zip(FIELDS, raw)]
    out = SpatialCorrelationDataset(class_result_labels(found), request, *raw, ocean.reshape(ny, nx), sdims,
                                    {d: np.asarray(coords[d]) for d in sdims if d in coords}, latv, dlon, shift, wraps,
                                    EARTH_RADIUS_KM, tdim, {"classes": classes if isinstance(classes, str) else "array"})
    return out
