"""detrend(): remove the long-term trend of every grid cell from the series BEFORE threshold() / detect() -- the
"shifting baseline" of the marine-heatwave literature (Jacox 2019; Amaya et al. 2023).  Neither xmhw nor
marineHeatWaves has it: users detrend on the host (numpy / xarray polyfit) and upload the result.  Here the fit
and the removal run on the resident device copy of the series (csrc/kernels_fit.hip).

The model, for one cell with samples y_t and a design matrix B[T][P] shared by all cells and built HERE, on the host:

* columns 0 .. R-1, the part that is REMOVED: x_t^k, k = 1..order, x_t = (time_t - t_ref) in decades of 3652.5 days
  (float64; datetime axes through nanoseconds as padding.interp_index does, numeric axes count days).  t_ref =
  ``reference`` if given, else the midpoint between the first and the last step of the fit period.  Every removed
  column is 0 at t_ref: the detrended series keeps the level it has there;
* columns R .. P-1, FITTED BUT KEPT: the constant 1, then cos(2 pi h phi_t), sin(2 pi h phi_t), h = 1..harmonics,
  phi_t = the time since t_ref in years of 365.25 days.  They are fitted jointly so that a seasonal cycle over a
  partial year or a gappy record does not leak into the trend; they stay because threshold() computes the climatology;
* order in {1, 2, 3}, harmonics in {0, 1, 2, 3}: P = order + 1 + 2 harmonics <= 10;
* a weight w_t in {0, 1} per step (the fit period); a NaN sample has weight 0 for its cell;
* beta = the least-squares solution over the contributing samples: normal equations in float64 in time order
  (sums of eight steps joined by compensated adds: csrc/kernels_fit.hip), Cholesky, two triangular solves, no FMA;
* a cell FAILS with fewer than max(min_valid, P) contributing samples, a contributing +-Inf, or a Cholesky pivot
  d_j = G_jj - sum_k L_jk^2 that is not > 1e-6 G_jj: all its coefficients and its whole detrended series are NaN --
  it drops out as land downstream, never a silently un-detrended cell;
* removal at EVERY step, inside or outside the fit period: y'_t = y_t - sum_{k<R} beta_k B[t][k], the sum in float64
  in column order, one subtraction, one rounding to the sample type.  NaN stays NaN.
"""
import numpy as np

from . import calendar as cal
from . import landmask
from .exception import XmhwException
from .padding import interp_index

MAX_TERMS = 10                         # include/xmhw_amd.h: XMHW_FIT_MAX_TERMS
_NS_PER_DAY = 86400.0e9
_DAYS_PER_DECADE = 3652.5
_DAYS_PER_YEAR = 365.25


def _abscissa(time):
    """(float64 abscissa, its units per day): nanoseconds for datetime axes, days for numeric ones; cftime-like
    objects become days since the first step"""
    t = np.asarray(time)
    if t.dtype == object and t.size and hasattr(t.flat[0], "year"):
        t0 = t.flat[0]
        t = np.array([(v - t0).total_seconds() / 86400.0 for v in t.flat], dtype=np.float64)
    try:
        x = interp_index(t)
    except (TypeError, ValueError) as e:
        raise XmhwException(f"detrend: {e}") from e
    return x, (_NS_PER_DAY if t.dtype.kind == "M" else 1.0)


def term_names(order, harmonics):
    names = [f"x{k}" for k in range(1, order + 1)] + ["const"]
    for h in range(1, harmonics + 1):
        names += [f"cos{h}", f"sin{h}"]
    return names


class DetrendSpec:
    """Design matrix, weights and parameters of one detrending, with their device copies made on first use (the shape
    of padding.PadSpec).  ``fitPeriod`` = [first, last]: years (inclusive) on a datetime / cftime axis, coordinate
    values on a numeric one; None leaves that end open.  ``reference``: a datetime64 (or a string numpy parses) on
    a datetime axis, a number on a numeric one."""

    def __init__(self, time, order=1, harmonics=2, fitPeriod=[None, None], reference=None, min_valid=None):
        if isinstance(order, bool) or order not in (1, 2, 3):
            raise XmhwException(f"detrend: order should be 1, 2 or 3, got {order!r}")
        if isinstance(harmonics, bool) or harmonics not in (0, 1, 2, 3):
            raise XmhwException(f"detrend: harmonics should be 0, 1, 2 or 3, got {harmonics!r}")
        if min_valid is not None and (isinstance(min_valid, bool) or int(min_valid) != min_valid or min_valid < 0):
            raise XmhwException(f"detrend: min_valid should be a non-negative integer, got {min_valid!r}")
        self.order, self.harmonics = int(order), int(harmonics)
        self.R = self.order
        self.P = self.order + 1 + 2 * self.harmonics
        self.terms = term_names(self.order, self.harmonics)
        self.min_valid = self.P if min_valid is None else max(int(min_valid), self.P)
        tv = np.asarray(time)
        if tv.ndim != 1 or tv.shape[0] == 0:
            raise XmhwException("detrend: the time axis is empty")
        self.x, per_day = _abscissa(tv)
        self.T = self.x.shape[0]
        self.datetime_axis = tv.dtype.kind == "M"
        first, last = (list(fitPeriod) + [None, None])[:2] if fitPeriod is not None else (None, None)
        w = np.ones(self.T, dtype=bool)
        if first is not None or last is not None:
            key = self.x if tv.dtype.kind in "fiu" else cal.years_of(tv)
            if first is not None:
                w &= key >= (float(first) if tv.dtype.kind in "fiu" else int(first))
            if last is not None:
                w &= key <= (float(last) if tv.dtype.kind in "fiu" else int(last))
        if not w.any():
            raise XmhwException(f"detrend: the fit period {list(fitPeriod)} selects no step of the time axis")
        self.fit_period = (first, last)
        self.weight = w.astype(np.uint8)
        idx = np.nonzero(w)[0]
        if reference is None:
            self.x_ref = 0.5 * (self.x[idx[0]] + self.x[idx[-1]])
        elif self.datetime_axis:
            try:
                self.x_ref = float(interp_index(np.array([np.datetime64(reference)]))[0])
            except (TypeError, ValueError) as e:
                raise XmhwException(f"detrend: reference {reference!r} is not a date") from e
        else:
            try:
                self.x_ref = float(reference)
            except (TypeError, ValueError) as e:
                raise XmhwException(f"detrend: reference {reference!r} is not a number") from e
        if self.datetime_axis:
            self.t_ref = np.datetime64("1970-01-01T00:00:00", "ns") + np.timedelta64(int(round(self.x_ref)), "ns")
        else:
            self.t_ref = self.x_ref
        days = (self.x - self.x_ref) / per_day
        xd = days / _DAYS_PER_DECADE
        phi = days / _DAYS_PER_YEAR
        B = np.empty((self.T, self.P), dtype=np.float64)
        for k in range(1, self.order + 1):
            B[:, k - 1] = xd ** k
        B[:, self.order] = 1.0
        for h in range(1, self.harmonics + 1):
            B[:, self.order + 2 * h - 1] = np.cos(2.0 * np.pi * h * phi)
            B[:, self.order + 2 * h] = np.sin(2.0 * np.pi * h * phi)
        self.basis = B
        self.all_steps = bool(w.all())
        self._dev = None

    def describe(self):
        """the provenance text of threshold_detect(detrend=...)"""
        return (f"series detrended before the climatology: order {self.order} polynomial in time removed, fitted "
                f"jointly with a constant and {self.harmonics} annual harmonics; fit period {list(self.fit_period)}; "
                f"reference time {self.t_ref}; a cell needs {self.min_valid} contributing samples")

    def _upload(self):
        from .device import DeviceBuffer
        if self._dev is None:
            self._dev = (DeviceBuffer.from_array(self.basis),
                         None if self.all_steps else DeviceBuffer.from_array(self.weight))
        return self._dev

    def apply(self, d_ts_ptr, itemsize, T, C, ld=None, stream=0, coef_out=None, nvalid_out=None):
        """Fit and remove, in place, on the device series (T, C).  ``coef_out`` / ``nvalid_out``: device pointers
        (or DeviceBuffers) that receive coef[P][C] float64 and nvalid[C] int32; without ``coef_out`` the
        coefficients live in a buffer of this call.  Returns the mask of the cells that FAILED (bool, C)."""
        from ._lib import hip
        from .device import DeviceScope, _ptr as ptr
        if T != self.T:
            raise ValueError("series and time axis differ in length")
        if C == 0 or T == 0:
            return np.zeros(C, dtype=bool)
        h = hip()
        d_basis, d_w = self._upload()
        with DeviceScope() as s:
            if coef_out is None:
                coef_out = s.alloc(8 * self.P * C)
            ld = int(C if ld is None else ld)
            h.series_fit(int(d_ts_ptr), int(itemsize), int(T), int(C), ld, d_basis.ptr, self.P,
                         d_w.ptr if d_w is not None else 0, self.min_valid, ptr(coef_out), int(C),
                         ptr(nvalid_out) if nvalid_out is not None else 0, stream)
            h.series_remove(int(d_ts_ptr), int(itemsize), int(T), int(C), ld, d_basis.ptr, self.P, self.R,
                            ptr(coef_out), int(C), stream)
            first = np.empty(C, dtype=np.float64)
            h.memcpy_d2h(first, ptr(coef_out), stream)          # the first coefficient row: NaN = failed (synchronises)
            return np.isnan(first)

    def free(self):
        if self._dev is not None:
            for b in self._dev:
                if b is not None:
                    b.free()
            self._dev = None


class SeriesRecipe:
    """What the device stages apply in place to every compacted slab between land_check and the climatology /
    detection kernels: maxPadLength's interpolation (padding.PadSpec, may be None), then the detrending.  Takes
    PadSpec's place in the ``pad`` argument of the device stages; ``apply`` returns the mask of the cells the
    detrending failed (they are NaN everywhere and the stage drops them like land)."""

    def __init__(self, pad, spec):
        self.pad, self.spec = pad, spec

    def apply(self, d_ts_ptr, itemsize, T, C, ld=None, stream=0):
        if self.pad is not None:
            self.pad.apply(d_ts_ptr, itemsize, T, C, ld, stream)
        return self.spec.apply(d_ts_ptr, itemsize, T, C, ld, stream)

    def free(self):                       # the DetrendSpec belongs to the caller that made it
        if self.pad is not None:
            self.pad.free()


def make_spec(detrend, time):
    """threshold_detect()'s ``detrend`` argument -> DetrendSpec (None: no detrending)"""
    if detrend is None or detrend is False:
        return None
    if detrend is True:
        return DetrendSpec(time)
    if not isinstance(detrend, dict):
        raise XmhwException("detrend should be None, True or a dict of detrend()'s keyword arguments")
    extra = set(detrend) - {"order", "harmonics", "fitPeriod", "reference", "min_valid"}
    if extra:
        raise XmhwException(f"detrend: unknown arguments {sorted(extra)}")
    return DetrendSpec(time, **detrend)


# ---- the device stages -----------------------------------------------------------------------------------------------
def detrend_cells_device(ts, spec, max_batch_bytes=32 << 30):
    """Device stage on a dense host (T, C) series: (detrended (T, C) of ts' dtype, coef (P, C), n_valid (C,))."""
    from ._lib import hip
    from .device import DeviceScope, native_float
    ts = np.ascontiguousarray(native_float(ts))
    T, C = ts.shape
    isz = ts.dtype.itemsize
    out = np.empty_like(ts)
    coef = np.empty((spec.P, C), dtype=np.float64)
    nvalid = np.empty(C, dtype=np.int32)
    cb = int(max(1, min(max(C, 1), max_batch_bytes // max(1, T * isz))))
    h = hip()
    for lo in range(0, C, cb):
        n = min(cb, C - lo)
        with DeviceScope() as s:
            d_ts = s.upload(np.ascontiguousarray(ts[:, lo:lo + n]))
            d_coef, d_nv = s.alloc(8 * spec.P * n), s.alloc(4 * n)
            spec.apply(d_ts.ptr, isz, T, n, coef_out=d_coef, nvalid_out=d_nv)
            h.stream_sync(0)
            out[:, lo:lo + n] = d_ts.to_array((T, n), ts.dtype)
            coef[:, lo:lo + n] = d_coef.to_array((spec.P, n), np.float64)
            nvalid[lo:lo + n] = d_nv.to_array((n,), np.int32)
    return out, coef, nvalid


def detrend_grid_device(stacked, spec, anynans, max_batch_bytes=None):
    """land_check() + detrending for an UNCOMPACTED stacked host series (T, N), slab by slab within the device
    budget: mask and compaction on the device as in threshold().  Returns (keep[N], detrended (T, N) with NaN at
    the dropped cells, coef (P, N) NaN there, n_valid (N,) 0 there)."""
    from ._lib import hip
    from .device import (DeviceScope, SlabPrefetcher, _grid_batch, device_itemsize, is_packed, mask_compact,
                         native_float)
    if is_packed(stacked):
        if stacked.ndim != 2 or stacked.strides[1] != stacked.dtype.itemsize:
            raise XmhwException("a file view must have contiguous rows (time, cells)")
    elif not (isinstance(stacked, np.ndarray) and stacked.dtype.kind == "f" and stacked.dtype.itemsize in (4, 8)
              and stacked.dtype.isnative and stacked.flags.c_contiguous):
        stacked = np.ascontiguousarray(native_float(stacked))
    T, N = stacked.shape
    isz = device_itemsize(stacked)
    dt = np.float32 if isz == 4 else np.float64
    h = hip()
    out = np.full((T, N), np.nan, dtype=dt)
    coef = np.full((spec.P, N), np.nan)
    nvalid = np.zeros(N, dtype=np.int32)
    keeps = []
    cb = _grid_batch(stacked, max_batch_bytes, per_cell_extra=8 * spec.P + 4)
    slabs = [(lo, min(N, lo + cb)) for lo in range(0, N, cb)]
    pre = SlabPrefetcher(stacked, slabs)
    try:
        for (lo, hi), (d_up, up_isz) in pre:
            d_ts, keep = mask_compact(d_up, up_isz, T, hi - lo, anynans)
            keeps.append(keep)
            if d_ts is None:
                continue
            n = int(keep.sum())
            with DeviceScope() as s:
                s.adopt(d_ts)
                d_coef, d_nv = s.alloc(8 * spec.P * n), s.alloc(4 * n)
                spec.apply(d_ts.ptr, isz, T, n, coef_out=d_coef, nvalid_out=d_nv)
                h.stream_sync(0)
                cols = lo + np.nonzero(keep)[0]
                if n == hi - lo:
                    h.memcpy2d_d2h(out, lo, n, d_ts.ptr)
                else:
                    out[:, cols] = d_ts.to_array((T, n), dt)
                coef[:, cols] = d_coef.to_array((spec.P, n), np.float64)
                nvalid[cols] = d_nv.to_array((n,), np.int32)
    finally:
        pre.close()
    keep = np.concatenate(keeps) if keeps else np.zeros(0, dtype=bool)
    if not keep.any():
        raise XmhwException("All points of grid are either land or NaN")
    return keep, out, coef, nvalid


class FitDataset:
    """The fit of detrend(): ``coef`` (term, *spatial dims) float64 with ``terms`` naming its rows ("x1", .., "const",
    "cos1", "sin1", ..), ``n_valid`` (spatial dims) the contributing samples of every cell, ``n_failed`` the number
    of ocean cells whose fit failed (NaN coefficients, NaN series), ``t_ref``, ``fit_period``.  ``dims`` are the
    non-time dims in sorted-name order (as land_check() stacks them); land cells are NaN."""

    def __init__(self, coef, terms, n_valid, n_failed, t_ref, fit_period, dims, coords, attrs):
        self.coef, self.terms, self.n_valid, self.n_failed = coef, list(terms), n_valid, int(n_failed)
        self.t_ref, self.fit_period = t_ref, tuple(fit_period)
        self.dims, self.coords, self.attrs = tuple(dims), coords, attrs

    def __getitem__(self, term):
        return self.coef[self.terms.index(term)]

    @property
    def trend_per_decade(self):
        return self.coef[self.terms.index("x1")]

    def to_xarray(self):
        import xarray as xr
        return xr.Dataset({"coef": (("term",) + self.dims, self.coef), "n_valid": (self.dims, self.n_valid)},
                          coords={"term": ("term", self.terms), **{k: (k, v) for k, v in self.coords.items()}},
                          attrs=dict(self.attrs))


def detrend(temp, tdim="time", order=1, harmonics=2, fitPeriod=[None, None], reference=None, anynans=False,
            min_valid=None):
    """Remove the per-cell polynomial trend (``order`` 1..3, per decade) of a temperature series, fitted jointly
    with a constant and ``harmonics`` annual harmonics over ``fitPeriod`` (module docstring).

    ``temp``: GridSeries, xarray.DataArray or a single-point (time-only) series.  Returns ``(detrended, fit)``:
    ``detrended`` has the input's type, dims, shape and floating dtype (other dtypes become float64); land cells
    (all NaN; any NaN with ``anynans``) and cells whose fit failed are NaN.  ``fit`` is a FitDataset.
    The device stage is always the HIP path (no CPU fallback)."""
    return _detrend(temp, detrend_cells_device, tdim, order, harmonics, fitPeriod, reference, anynans, min_valid,
                    grid_compute=detrend_grid_device)


def _detrend(temp, compute, tdim="time", order=1, harmonics=2, fitPeriod=[None, None], reference=None, anynans=False,
             min_valid=None, grid_compute=None):
    """Host side of detrend() around a device stage ``compute`` (signature of detrend_cells_device) and, for grids,
    ``grid_compute`` (signature of detrend_grid_device); the CPU tests pass numpy stand-ins."""
    from .api import GridSeries, _from_xarray, _is_xarray
    is_xr = _is_xarray(temp)
    dims = list(temp.dims)
    if tdim not in dims:
        raise XmhwException(f"{tdim} dimension not present, default"
                            + "is 'time' or pass as tdim='time_dimension_name'")
    if is_xr:
        values = temp.values
        coords, _ = _from_xarray(temp)
    else:
        values, coords = temp.values, dict(temp.coords)
    time = np.asarray(coords[tdim])
    spec = DetrendSpec(time, order, harmonics, fitPeriod, reference, min_valid)
    tax = dims.index(tdim)
    point = len(dims) == 1
    try:
        if point:
            out, coef, nvalid = compute(np.ascontiguousarray(np.asarray(values).reshape(-1, 1)), spec)
            keep, sdims, sshape = np.array([True]), [], ()
        elif grid_compute is not None:
            stacked, sdims, sshape = landmask.stack_cells(values, dims, tdim)
            keep, out, coef, nvalid = grid_compute(stacked, spec, anynans)
        else:
            ts, keep, sdims, sshape = landmask.land_check(values, dims, tdim, anynans)
            o, c, n = compute(ts, spec)
            out = np.full((o.shape[0], keep.shape[0]), np.nan, dtype=o.dtype)
            coef = np.full((spec.P, keep.shape[0]), np.nan)
            nvalid = np.zeros(keep.shape[0], dtype=np.int32)
            out[:, keep], coef[:, keep], nvalid[keep] = o, c, n
    finally:
        spec.free()
    T = time.shape[0]
    n_failed = int((np.isnan(coef[0]) & keep).sum())
    # back to the input's layout: (time, *sorted dims) -> the input's order of dims
    order_now = [tdim] + list(sdims)
    grid = out.reshape((T,) + tuple(sshape))
    grid = np.transpose(grid, [order_now.index(d) for d in dims])
    fit = FitDataset(coef.reshape((spec.P,) + tuple(sshape)), spec.terms, nvalid.reshape(tuple(sshape)), n_failed,
                     spec.t_ref, spec.fit_period, sdims, {d: np.asarray(coords[d]) for d in sdims},
                     {"order": spec.order, "harmonics": spec.harmonics, "min_valid": spec.min_valid,
                      "t_ref": str(spec.t_ref), "fit_period": str(list(spec.fit_period)),
                      "trend_units": "per decade of 3652.5 days"})
    if is_xr:
        detrended = temp.copy(data=grid)
    else:
        detrended = GridSeries(grid, temp.dims, temp.coords, attrs=temp.attrs, coord_attrs=temp.coord_attrs,
                               time_encoding=temp.time_encoding)
    return detrended, fit
