"""coarsen(): weighted block means in space and time -- the front-end stage: daily series to pentad or monthly means, a
0.05 degree tile to the 0.25 degree grid of a climatology, the series under maximum_monthly_mean(), a coarse first look
before a full-resolution run, and the grid under the reach of spatial_correlation() or the lag range of
lag_correlation().  Its output is an ordinary series: it goes into threshold(), detect(), threshold_detect() and every
analysis stage as it is.  One pass over the UNCOMPACTED grid in time blocks, every sample read once
(csrc/kernels_coarsen.hip, csrc/coarsen_index.h).

The definition (include/xmhw_amd.h, "coarsen()", states it for the C entries).  Inputs: the fine series x[t, j, i],
uncompacted on the ny x nx grid, longitude the fast axis, float32 or float64, NaN = no sample; int32 weights wi[j, i],
0 <= wi <= 2**24; factors fy, fx >= 1; a coarse grid ncy x ncx, ncy <= ceil(ny / fy), ncx <= ceil(nx / fx) (a block that
hangs over the grid holds only its in-grid points); windows [t0, t1) of steps.  For the coarse entry (s, J, I), over the
in-grid fine samples of block x window that have wi > 0 and are not NaN:
    xq = rint((float64(x) - x0) * 2**16)             (the fixed point of region_series(), in float64 as written)
    a sample with |x - x0| >= 2**7, or infinite, is left out of all sums and counted (n_range)
    n += 1, wsum += wi, xsum += wi * xq               (exact integers)
W = the sum of wi over the in-grid points of the block, land included; len = the window's length.  The entry is VALID iff
n >= 1 and wsum * 65536 >= a * len * W, a an integer in [0, 65536]: the least covered share in 65536ths, equality counts
as valid.  The value is x0 + (float64(xsum) / float64(wsum)) / 65536.0 in float64 as written, rounded once to the sample
type; an invalid entry is NaN.  fy * fx * (the longest window) <= 4096: then |xsum| <= 2**59, wsum * 65536 < 2**52 and
a * len * W <= 2**52.  Every sum is an integer sum and the finish is two conversions, one correctly rounded division, an
exact scaling and one add: the result does not depend on launch geometry, time blocks or load widths, and numpy
reproduces every bit.

Host side here (factors, windows, weights, coordinates, time blocks); device side behind coarsen_grid().
"""
import numpy as np

from ._lib import hip, hip_coarsen
from .device import DeviceScope, as_xmhw_errors, device_budget_bytes, is_packed, native_float
from .exception import XmhwException
from .gridweights import quantise_weights, resolve_weights, weights_label
from .series_stage import grid_layout

MAX_VOLUME = 4096               # XMHW_COARSEN_MAX_VOLUME (include/xmhw_amd.h)
WEIGHT_BITS = 24                # XMHW_COARSEN_MAX_WEIGHT_BITS
BITS = 16                       # XMHW_REGION_SERIES_BITS
RANGE_BITS = 7                  # |x - offset| < 2**7
SHARE_ONE = 65536               # min_fraction is taken in 65536ths
BOUNDARIES = ("trim", "pad")
TIME_LABELS = ("left", "center")
CALENDAR_UNITS = ("month", "year")


# ---- factors, windows, the coarse grid ---------------------------------------------------------------

def _whole(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
        raise XmhwException(f"{what} should be a whole number >= 1, got {v!r}")
    return int(v)


def check_space(space, sdims):
    """``space`` as (fy, fx) on the stacked (sorted-name) spatial dims ``sdims`` (none, one -- then fy = 1 -- or two):
    None = (1, 1); an int = that factor on every spatial dim; a pair (slow, fast) in stacked order; a dict by dim name"""
    nd = len(sdims)
    if nd > 2:
        raise XmhwException(f"coarsen handles one or two spatial dims, got {list(sdims)}")
    if space is None:
        f = [1] * nd
    elif isinstance(space, dict):
        unknown = [k for k in space if k not in sdims]
        if unknown:
            raise XmhwException(f"space names {unknown}, which are no spatial dims of the series ({list(sdims)})")
        f = [_whole(space.get(d, 1), f"space[{d!r}]") for d in sdims]
    elif isinstance(space, (int, np.integer)) and not isinstance(space, bool):
        f = [_whole(space, "space")] * nd
    else:
        try:
            f = [_whole(v, "a factor of space") for v in space]
        except TypeError:
            raise XmhwException(f"space should be None, a whole number, a pair (slow, fast) or a dict by dim name, got "
                                f"{space!r}") from None
        if len(f) != nd:
            raise XmhwException(f"space should hold one factor per spatial dim {list(sdims)}, got {space!r}")
    if nd == 0 and space not in (None, 1):
        raise XmhwException("a time-only series has no spatial dim to coarsen: pass space=None")
    return tuple([1] * (2 - nd) + f)


def check_windows(T, time=None, windows=None, boundary="trim"):
    """(S, 2) int32 windows [start, stop) of the T steps: ``time`` = n gives consecutive windows of n steps from step 0
    (a partial last one is dropped under "trim" and kept, shorter, under "pad"); ``windows`` is an increasing array of
    S + 1 boundaries (window s = [w[s], w[s + 1])) or an (S, 2) array of [start, stop) pairs in increasing order, which
    may leave steps uncovered between them; neither: windows of one step"""
    if boundary not in BOUNDARIES:
        raise XmhwException(f"boundary should be one of {BOUNDARIES}, got {boundary!r}")
    if time is not None and windows is not None:
        raise XmhwException("pass time or windows, not both")
    T = int(T)
    if windows is None:
        n = 1 if time is None else _whole(time, "time")
        edges = np.arange(0, T + 1, n, dtype=np.int64)
        if boundary == "pad" and edges[-1] < T:
            edges = np.append(edges, T)
        pairs = np.stack([edges[:-1], edges[1:]], axis=1)
    else:
        w = np.asarray(windows)
        if w.dtype.kind not in "iu" or w.ndim not in (1, 2) or (w.ndim == 2 and w.shape[1] != 2) or (w.ndim == 1 and w.size < 1):
            raise XmhwException("windows should be an increasing array of S + 1 whole-number boundaries or an (S, 2) array "
                                f"of [start, stop) pairs, got {windows!r}")
        w = w.astype(np.int64)
        pairs = np.stack([w[:-1], w[1:]], axis=1) if w.ndim == 1 else w
        flat = pairs.reshape(-1)
        if pairs.shape[0] and ((pairs[:, 1] <= pairs[:, 0]).any() or (pairs[1:, 0] < pairs[:-1, 1]).any()):
            raise XmhwException("windows should be strictly increasing: every window holds a step and none overlaps the next")
        if flat.size and (flat[0] < 0 or flat[-1] > T):
            raise XmhwException(f"windows should lie in [0, {T}], the steps of the series, got {int(flat[0])} .. {int(flat[-1])}")
    return np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)


def calendar_windows(time_axis, unit):
    """The boundaries (S + 1,) int64 of the calendar periods present in ``time_axis`` (datetime64, ascending), ``unit``
    "month" or "year", for ``coarsen(windows=...)``.  The first and the last period are returned as they are: where the
    record starts or ends inside a period that window is a partial month or year -- trim it (``w[1:]``, ``w[:-1]``)."""
    if unit not in CALENDAR_UNITS:
        raise XmhwException(f"unit should be one of {CALENDAR_UNITS}, got {unit!r}")
    t = np.asarray(time_axis)
    if t.dtype.kind != "M" or t.ndim != 1 or t.size < 1:
        raise XmhwException("calendar_windows needs a datetime64 time axis with a step at least")
    period = t.astype("datetime64[M]" if unit == "month" else "datetime64[Y]").astype(np.int64)
    if (np.diff(period) < 0).any():
        raise XmhwException("the time axis should be ascending")
    return np.concatenate([[0], np.nonzero(np.diff(period))[0] + 1, [t.size]]).astype(np.int64)


def coarse_cells(n, f, boundary):
    """the cells of an axis of n points under the factor f: "trim" drops a partial last block, "pad" keeps it"""
    return -(-int(n) // int(f)) if boundary == "pad" else int(n) // int(f)


def check_share(min_fraction):
    """a = rint(min_fraction * 65536), the least covered share in 65536ths"""
    try:
        f = float(min_fraction)
    except (TypeError, ValueError):
        f = np.nan
    if not 0.0 <= f <= 1.0:
        raise XmhwException(f"min_fraction should be in [0, 1], got {min_fraction!r}")
    return int(np.rint(f * SHARE_ONE))


def check_volume(fy, fx, win):
    """fy * fx * (the longest window) <= 4096 samples: the bound behind the 64 bits of xsum"""
    longest = int((win[:, 1] - win[:, 0]).max()) if win.shape[0] else 1
    if fy * fx * longest > MAX_VOLUME:
        raise XmhwException(f"a block of {fy} x {fx} points over a window of {longest} steps holds {fy * fx * longest} "
                            f"samples, more than {MAX_VOLUME}: coarsen in two passes (space, then time)")


def block_weight(wi, ny, nx, fy, fx, ncy, ncx):
    """W (ncy, ncx) int64: the sum of wi over the in-grid points of every block"""
    hy, hx = min(ny, ncy * fy), min(nx, ncx * fx)
    w = np.pad(np.asarray(wi, dtype=np.int64).reshape(ny, nx)[:hy, :hx], ((0, ncy * fy - hy), (0, ncx * fx - hx)))
    return w.reshape(ncy, fy, ncx, fx).sum(axis=(1, 3))


def block_mean_coord(coord, f, nc):
    """(nc,) float64: the mean of the in-grid fine coordinates of every block of f points"""
    c = np.asarray(coord, dtype=np.float64)
    return np.array([c[k * f:min((k + 1) * f, c.size)].mean() for k in range(nc)], dtype=np.float64)


# ---- the device stage --------------------------------------------------------------------------------

def check_stage_inputs(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win):
    """What both stages (the device's and a stand-in) may rely on: the arguments checked as the C entries check them and
    in the layouts the device takes; windows as (S, 2) [start, stop) pairs"""
    if is_packed(field):
        raise XmhwException("coarsen does not read packed int16 views: pass decoded floats")
    field = np.ascontiguousarray(native_float(np.asarray(field)))
    ny, nx, fy, fx, ncy, ncx = (int(v) for v in (ny, nx, fy, fx, ncy, ncx))
    if ny < 1 or nx < 1 or ny * nx >= 2 ** 31:
        raise XmhwException(f"coarsen handles grids of 1 to 2**31 - 1 points, got {ny} x {nx}")
    if field.ndim != 2 or field.shape[1] != ny * nx:
        raise XmhwException(f"the series should be (T, {ny * nx}) on the {ny} x {nx} grid, got {field.shape}")
    if fy < 1 or fx < 1:
        raise XmhwException(f"the factors should be >= 1, got ({fy}, {fx})")
    if not (0 <= ncy <= -(-ny // fy) and 0 <= ncx <= -(-nx // fx)):
        raise XmhwException(f"the coarse grid {ncy} x {ncx} is no coarse grid of {ny} x {nx} under ({fy}, {fx})")
    wi = np.ascontiguousarray(wi)
    if wi.shape != (ny * nx,) or wi.dtype.kind not in "iu" or (wi.size and (wi.min() < 0 or wi.max() > 1 << WEIGHT_BITS)):
        raise XmhwException(f"wi should hold one whole number in [0, 2**{WEIGHT_BITS}] per grid point")
    win = check_windows(field.shape[0], windows=np.asarray(win))
    check_volume(fy, fx, win)
    x0, a = float(x0), int(a)
    if not np.isfinite(x0):
        raise XmhwException(f"offset should be a finite number, got {x0}")
    if not 0 <= a <= SHARE_ONE:
        raise XmhwException(f"a should be in [0, {SHARE_ONE}], got {a}")
    return field, ny, nx, fy, fx, ncy, ncx, wi.astype(np.int32), x0, a, win


def window_blocks(win, row_bytes, budget, block_steps=None):
    """[(first window, windows)]: the windows in time blocks that are unions of whole windows: a block's rows (from its
    first window's start to its last one's stop) fit ``budget`` bytes, or ``block_steps`` steps; one window at least"""
    most = int(block_steps) if block_steps else int(max(1, budget // max(row_bytes, 1)))
    if most < 1:
        raise XmhwException("block_steps should be >= 1")
    out, s = [], 0
    while s < win.shape[0]:
        e = s + 1
        while e < win.shape[0] and win[e, 1] - win[s, 0] <= most:
            e += 1
        out.append((s, e - s))
        s = e
    return out


def _runs(win):
    """[(first, count)] over the windows: the runs of windows that follow each other without a gap (one C call each)"""
    cut = np.nonzero(win[1:, 0] != win[:-1, 1])[0] + 1
    edges = [0] + [int(c) for c in cut] + [win.shape[0]]
    return [(edges[k], edges[k + 1] - edges[k]) for k in range(len(edges) - 1)]


def coarsen_grid(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win, want=False, max_batch_bytes=None, block_steps=None):
    """The device stage.  ``field`` (T, ny * nx): the UNCOMPACTED host series, float32 or float64; ``wi`` (ny * nx,) whole
    numbers in [0, 2**24]; ``win`` the windows as S + 1 boundaries or (S, 2) [start, stop) pairs.  Returns
    (out (S, ncy * ncx) in the dtype of the series, wsum int64 and n int32 likewise or None without ``want``, n_range).
    The series goes through the device in time blocks that are unions of whole windows, below ``max_batch_bytes`` (or of
    ``block_steps`` steps at most, one window at least): upload the fine block, queue the kernel, download the coarse
    block, free the fine block; the weights stay resident.  The blocks do not change a bit.  Out-of-range samples are
    counted, not refused, here."""
    field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win = check_stage_inputs(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win)
    S, cells, N = win.shape[0], ncy * ncx, ny * nx
    isz = field.dtype.itemsize
    out = np.full((S, cells), np.nan, dtype=field.dtype)
    wsum = np.zeros((S, cells), dtype=np.int64) if want else None
    n = np.zeros((S, cells), dtype=np.int32) if want else None
    if S == 0 or cells == 0:
        return out, wsum, n, 0
    h, hc = hip(), hip_coarsen()
    if max_batch_bytes is None:
        max_batch_bytes = device_budget_bytes()
    with DeviceScope() as resident:
        d_wi = resident.upload(wi)
        d_range = resident.upload(np.zeros(1, dtype=np.int64))
        budget = max(int(max_batch_bytes) - 4 * N, 0)
        for s0, count in window_blocks(win, N * isz, budget, block_steps):
            t0, t1 = int(win[s0, 0]), int(win[s0 + count - 1, 1])
            with DeviceScope() as s:
                d_ts = s.upload(field[t0:t1])
                d_out = s.alloc(count * cells * isz)
                d_wsum = s.alloc(count * cells * 8) if want else None
                d_n = s.alloc(count * cells * 4) if want else None
                for r0, rc in _runs(win[s0:s0 + count]):
                    table = np.append(win[s0 + r0:s0 + r0 + rc, 0], win[s0 + r0 + rc - 1, 1]).astype(np.int32) - t0
                    with as_xmhw_errors(also="Unsupported"):
                        hc.coarsen(d_ts.ptr, isz, t1 - t0, N, ny, nx, fy, fx, ncy, ncx, d_wi.ptr, x0, a, table,
                                   d_out.ptr + r0 * cells * isz, cells, d_wsum.ptr + r0 * cells * 8 if want else 0,
                                   d_n.ptr + r0 * cells * 4 if want else 0, d_range.ptr)
                h.stream_sync(0)
                out[s0:s0 + count] = d_out.to_array((count, cells), field.dtype)
                if want:
                    wsum[s0:s0 + count] = d_wsum.to_array((count, cells), np.int64)
                    n[s0:s0 + count] = d_n.to_array((count, cells), np.int32)
        n_range = int(d_range.to_array((1,), np.int64)[0])
    return out, wsum, n, n_range


# ---- the result --------------------------------------------------------------------------------------

class CoarsenInfo:
    """What coarsen() says about its result, as plain arrays.

    factors {dim: factor} of the spatial dims, sdims and the coarse coords; windows (S, 2) int32 the [start, stop) steps
    of every coarse step; boundary, time_label, offset; a = the least covered share in 65536ths; weight_unit = w.max() /
    2**24 (an integer weight times it is in the units of the weights); n_range = 0 (the call raises otherwise);
    coverage float32 (S, ncy, ncx) = wsum / (len * W), the share of the block x window's weight that had a sample (NaN
    for a block without weight) -- filled only with ``coverage=True``, else None -- with wsum int64 and n int32 beside it."""

    def __init__(self, factors, sdims, coords, windows, boundary, time_label, offset, a, weight_unit, n_range, dtype,
                 coverage=None, wsum=None, n=None, tdim="time", time=None, attrs=None):
        self.factors, self.sdims, self.coords = dict(factors), tuple(sdims), dict(coords)
        self.windows = np.asarray(windows, dtype=np.int32).reshape(-1, 2)
        self.boundary, self.time_label, self.offset, self.a = boundary, time_label, float(offset), int(a)
        self.weight_unit, self.n_range, self.dtype = float(weight_unit), int(n_range), np.dtype(dtype)
        self.coverage, self.wsum, self.n = coverage, wsum, n
        self.tdim, self.time, self.attrs = tdim, time, dict(attrs or {})

    def quantisation_bound(self, values):
        """A bound on |coarse - the weighted mean of the samples as float64 under the integer weights|, like ``values``
        (the coarse series): 2**-17, the half unit by which a sample's fixed point is off, plus half an ulp of the
        output type at the value, its one rounding.  (The float64 finish adds less than 2**-44.)  NaN where the value is."""
        v = np.asarray(values)
        half_ulp = 0.5 * np.spacing(np.abs(v.astype(self.dtype))).astype(np.float64)
        return 2.0 ** -(BITS + 1) + half_ulp

    def to_xarray(self):
        import xarray as xr
        data = {"windows": (("step", "edge"), self.windows)}
        coords = {d: self.coords[d] for d in self.sdims if d in self.coords}
        if self.coverage is not None:
            dims = (self.tdim,) + self.sdims
            data.update(coverage=(dims, self.coverage), wsum=(dims, self.wsum), n=(dims, self.n))
            if self.time is not None:
                coords[self.tdim] = self.time
        return xr.Dataset(data, coords=coords,
                          attrs=dict(self.attrs, boundary=self.boundary, time_label=self.time_label, offset=self.offset,
                                     min_share_65536ths=self.a, weight_unit=self.weight_unit, n_range=self.n_range,
                                     **{f"factor_{d}": f for d, f in self.factors.items()}))


# ---- the public function -----------------------------------------------------------------------------

def _window_stamps(time, win, time_label):
    """the time coordinate of the coarse steps: a window's first stamp ("left"), or the midpoint of its first and last"""
    first, last = time[win[:, 0]], time[win[:, 1] - 1]
    if time_label == "left":
        return first
    if time.dtype.kind == "M":
        return first + (last - first) // 2
    return np.array([a + (b - a) / 2 for a, b in zip(first, last)], dtype=time.dtype)


def coarsen(temp, space=None, time=None, windows=None, weights=None, min_fraction=0.5, boundary="trim", offset=0.0,
            time_label="left", tdim="time", max_batch_bytes=None, block_steps=None, coverage=False, _compute=None):
    """Weighted block means of a series in space and time.

    ``temp``: a GridSeries, an xarray.DataArray or a time-only series, with one or two spatial dims in the stacked
    (sorted-name) order of landmask.stack_cells (one dim: a grid of one row); samples are read as stored, packed int16
    views are refused.  ``space``: the spatial factors -- None = (1, 1), a whole number, a pair (slow, fast) in stacked
    order or a dict by dim name.  ``time`` = n: consecutive windows of n steps from step 0; ``windows``: an increasing
    array of S + 1 boundaries, or (S, 2) [start, stop) pairs that may leave steps uncovered between them (gaps);
    time or windows, not both; neither: windows of one step.  calendar_windows(time_axis, "month" | "year") gives the
    boundaries of the calendar periods.  ``boundary``: "trim" drops partial trailing blocks and a partial trailing
    ``time=n`` window; "pad" keeps them, and coverage is then relative to what the grid and the record hold (a partial
    last column leaves the coarse longitude non-uniform: the stages that need a uniform longitude refuse that output).
    ``weights``: None, "coslat" or an array on the spatial grid (gridweights.resolve_weights), quantised to 24 bits.
    ``min_fraction`` in [0, 1]: the least share of a block x window's weight (land included) that must have had a sample,
    taken in 65536ths, a = rint(min_fraction * 65536); a block at exactly that share is valid.  ``offset``: x0 of the
    definition; |temp - offset| must stay below 2**7 (``offset=273.15`` for kelvin), else the call raises.
    fy * fx * (the longest window) <= 4096 samples.

    Returns ``(coarse, info)``: ``coarse`` has the type, the dims and the floating dtype of the input (other dtypes become
    float64); a coarse spatial coordinate is the float64 mean of the block's in-grid fine coordinates, the time
    coordinate the window's first stamp (``time_label="left"``) or the midpoint of its first and last stamps
    ("center").  ``info`` is a CoarsenInfo; ``coverage=True`` fills its coverage, wsum and n.  ``block_steps``: the steps
    of a time block on the device at most (None: what fits ``max_batch_bytes``); blocks are unions of whole windows and
    change no bit.  ``_compute``: a stand-in for coarsen_grid() (host tests)."""
    from .api import GridSeries, _is_xarray
    from .landmask import stack_cells
    if time_label not in TIME_LABELS:
        raise XmhwException(f"time_label should be one of {TIME_LABELS}, got {time_label!r}")
    if boundary not in BOUNDARIES:
        raise XmhwException(f"boundary should be one of {BOUNDARIES}, got {boundary!r}")
    a = check_share(min_fraction)
    offset = float(offset)
    if not np.isfinite(offset):
        raise XmhwException(f"offset should be a finite number, got {offset}")
    coords, _, dims, point, sdims, sshape, N = grid_layout(temp, tdim)
    fy, fx = check_space(space, sdims)
    values = temp.values
    if is_packed(values):
        raise XmhwException("coarsen does not read packed int16 views: pass decoded floats")
    ny, nx = ([1] * (2 - len(sshape)) + [int(v) for v in sshape])
    taxis = np.asarray(coords[tdim])
    T = int(taxis.shape[0])
    win = check_windows(T, time, windows, boundary)
    check_volume(fy, fx, win)
    ncy, ncx = coarse_cells(ny, fy, boundary), coarse_cells(nx, fx, boundary)
    if ncy < 1 or ncx < 1 or win.shape[0] < 1:
        raise XmhwException(f"nothing is left of {ny} x {nx} points x {T} steps under the factors ({fy}, {fx}), the windows "
                            f"and boundary={boundary!r}: use smaller factors or boundary='pad'")
    w = resolve_weights(weights, coords, dims, tdim, sdims, sshape, point)
    wq, unit = quantise_weights(w, WEIGHT_BITS)
    field = np.asarray(values).reshape(-1, 1) if point else stack_cells(np.asarray(values), dims, tdim)[0]
    stage = _compute or coarsen_grid
    out, wsum, n, n_range = stage(field, ny, nx, fy, fx, ncy, ncx, wq.astype(np.int32), offset, a, win, want=bool(coverage),
                                  max_batch_bytes=max_batch_bytes, block_steps=block_steps)
    S, cells = win.shape[0], ncy * ncx
    out = np.asarray(out)
    if out.shape != (S, cells):
        raise XmhwException(f"coarsen stage returned {out.shape}, expected {(S, cells)}")
    if n_range:
        raise XmhwException(f"{int(n_range)} samples lie 2**{RANGE_BITS} and more from offset={offset} (or are infinite): "
                            "pass offset=273.15 for a series in kelvin")
    # the coarse frame: coordinates, then the input's order of dims
    factor_of = dict(zip(sdims, (fy, fx)[2 - len(sdims):]))
    count_of = dict(zip(sdims, (ncy, ncx)[2 - len(sdims):]))
    new_coords = {tdim: _window_stamps(taxis, win, time_label)}
    for d in sdims:
        if d in coords:
            c = np.asarray(coords[d])
            new_coords[d] = block_mean_coord(c, factor_of[d], count_of[d]) if c.dtype.kind in "fiu" else c[::factor_of[d]][:count_of[d]]
    cshape = tuple(count_of[d] for d in sdims)
    order_now = [tdim] + list(sdims)
    to_input = [order_now.index(d) for d in dims]
    grid = np.transpose(out.reshape((S,) + cshape), to_input)
    cov = None
    if coverage:
        W = block_weight(wq, ny, nx, fy, fx, ncy, ncx).reshape(-1)
        length = (win[:, 1] - win[:, 0]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            cov = (np.asarray(wsum).astype(np.float64) / (length[:, None] * W[None].astype(np.float64))).astype(np.float32)
        cov = cov.reshape((S,) + cshape)
        wsum, n = np.asarray(wsum).reshape((S,) + cshape), np.asarray(n).reshape((S,) + cshape)
    info = CoarsenInfo(factor_of, sdims, {d: new_coords[d] for d in sdims if d in new_coords}, win, boundary, time_label,
                       offset, a, unit, n_range, out.dtype, cov, wsum if coverage else None, n if coverage else None, tdim,
                       new_coords[tdim], {"weights": weights_label(weights)})
    if _is_xarray(temp):
        import xarray as xr
        tcoord = xr.Variable((tdim,), new_coords[tdim], attrs=dict(temp[tdim].attrs))
        tcoord.encoding = dict(getattr(temp[tdim], "encoding", {}) or {})
        xc = {tdim: tcoord}
        xc.update({d: xr.Variable((d,), new_coords[d], attrs=dict(temp[d].attrs)) for d in sdims if d in temp.coords})
        coarse = xr.DataArray(grid, dims=temp.dims, coords=xc, attrs=dict(temp.attrs), name=temp.name)
    else:
        coarse = GridSeries(grid, temp.dims, {d: new_coords[d] for d in dims if d in new_coords}, attrs=temp.attrs,
                            coord_attrs=temp.coord_attrs, time_encoding=temp.time_encoding)
    return coarse, info
