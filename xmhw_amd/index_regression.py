"""index_regression(): lagged regression and correlation maps of the anomalies of every cell on climate indices -- what
drives the heatwaves of a cell (Holbrook et al. 2019; Sen Gupta et al. 2020).  For every cell the anomaly
a = temp - base is regressed on an index (Nino-3.4, the IOD box, a basin mean: ``region_series().series()`` builds them
on the device) that leads by 0, 30, 60 ... steps, per class of time steps (``classes="season"``; the phases of
``classes_from_events()``), and the correlation comes with the effective sample size that daily, strongly autocorrelated
series need.  One streaming pass over the series (csrc/kernels_regress.hip): a small matrix product,
cells x time against time x predictors, in exact 64-bit integers.

The device sums.  ``class_of_t``: one int32 label per step in [-1, K), -1 = the step counts nowhere.  ``zq`` (T, J)
int32: the predictor table in fixed point, |zq| < 2**23.  With a = float64(sample) - base[row(t), c], a step is VALID
iff a is not NaN and |a| < 2**7, and q(t) = rint(a * 2**16) on valid steps.  Per class k and cell c:
    n[k, c]      (int32)   valid steps of class k
    sa[k, c]     (int64)   sum of q over them
    saa[k, c]    (int64)   sum of q**2 over them
    n1[k, c]     (int32)   valid steps t >= 1 of class k whose step t - 1 is valid and of class k as well
    saa1[k, c]   (int64)   sum of q(t) q(t - 1) over those
    saz[k, j, c] (int64)   sum of q(t) zq[t, j] over the valid steps of class k
    mz[k, j, c]  (int64)   sum of zq[t, j] over the steps of class k that are NOT valid (NaN or out of range)
    mzz[k, j, c] (int64)   sum of zq[t, j]**2 over those
Any non-NaN a with |a| >= 2**7 is left out and counted in n_range (index_regression() raises if n_range > 0).  mz and
mzz are deficits: the sums of zq and zq**2 over the cell's own valid steps are the class totals, computed here once,
minus them.  Everything is an integer sum: the result does not depend on the time blocks, the slabs, the launch
geometry or the schedule.

Host side here (validation, predictor table, class labels, slabs, land, derived fields); device side behind
regress_cells() (a compact host series) and regress_grid() (a stacked grid, masked and compacted on the device).
"""
import numpy as np

from ._lib import hip_regress
from .device import as_xmhw_errors
from .exception import XmhwException
from .series_stage import (Accumulators, base_series, cell_stage, check_class_ids, check_steps, class_labels,
                           class_result_labels, dense_ids, grid_layout, run_cells, run_grid, stage_attrs)
from .trend import p_two_sided

MAX_PREDICTORS = 32             # XMHW_INDEX_REGRESS_MAX_PREDICTORS (include/xmhw_amd.h)
MAX_CLASSES = 64                # XMHW_INDEX_REGRESS_MAX_CLASSES
MAX_STEPS = 1 << 17             # XMHW_INDEX_REGRESS_MAX_STEPS: T below it
BITS = 16                       # XMHW_INDEX_REGRESS_BITS
RANGE_BITS = 7                  # |a| < 2**7, |z| < 2**7
_ONE = float(1 << BITS)
_ZLIM = 1 << (BITS + RANGE_BITS)                # |zq| < 2**23
_RANGE_TEXT = ("samples lie 2**7 and more from their base (or are infinite): is the series in kelvin and the base in "
               "degrees Celsius?")
FIELDS = ("n", "sa", "saa", "n1", "saa1", "saz", "mz", "mzz")
_PER_CELL = FIELDS[:5]                          # (K, C); the rest are per predictor as well, (K, J, C)


# ---- validation (mirrors the refusals of the C entries) ----------------------------------------------

def check_regress_arguments(T, classes, K, zq):
    """The stage-side check: (classes int32 (T,), K, zq int32 (T, J))"""
    check_steps(T, "index_regression")
    classes, K = check_class_ids(T, classes, K, MAX_CLASSES, "index_regression")
    zq = np.asarray(zq)
    if zq.ndim != 2 or zq.shape[0] != T or zq.dtype.kind not in "iu":
        raise XmhwException(f"zq should be a ({T}, J) integer table, got {zq.dtype} {zq.shape}")
    if not 1 <= zq.shape[1] <= MAX_PREDICTORS:
        raise XmhwException(f"index_regression handles 1 to {MAX_PREDICTORS} predictors, got {zq.shape[1]}")
    if zq.size and np.abs(zq.astype(np.int64)).max() >= _ZLIM:
        raise XmhwException("quantised predictors should lie inside (-2**23, 2**23)")
    return classes, K, np.ascontiguousarray(zq, dtype=np.int32)


def _index_values(name, x, T):
    """one index as float64 (T,): an array, or a (time, 1) series such as a one-region region_series().series()"""
    x = np.asarray(x.values if hasattr(x, "values") else x, dtype=np.float64)
    if x.ndim == 2 and x.shape[1] == 1:
        x = x[:, 0]
    if x.shape != (T,):
        raise XmhwException(f"index {name!r} should have one value per time step ({T}), got shape {x.shape}")
    return x


def check_lags(lags):
    lags = np.atleast_1d(np.asarray(lags))
    if lags.ndim != 1 or lags.size == 0 or lags.dtype.kind not in "iu":
        raise XmhwException("lags should be a sequence of whole numbers of steps")
    if np.unique(lags).shape[0] != lags.shape[0]:
        raise XmhwException("lags should be distinct")
    return lags.astype(np.int64)


def lagged_predictors(indices, lags, T):
    """(names, lags, X): X float64 (T, I, L) with X[t, i, l] = x_i(t - lags[l]) -- a positive lag means that the index
    leads -- and NaN where the index is missing or t - lag falls off the axis."""
    if not isinstance(indices, dict) or not indices:
        raise XmhwException("indices should be a non-empty dict from name to a series of length T")
    lags = check_lags(lags)
    names = tuple(indices)
    if len(names) * lags.shape[0] > MAX_PREDICTORS:
        raise XmhwException(f"index_regression handles at most {MAX_PREDICTORS} predictors (indices x lags), got "
                            f"{len(names)} x {lags.shape[0]}")
    X = np.full((T, len(names), lags.shape[0]), np.nan)
    for i, name in enumerate(names):
        x = _index_values(name, indices[name], T)
        if np.isinf(x).any():
            raise XmhwException(f"index {name!r} holds infinite values")
        for l, lag in enumerate(lags):
            lag = int(lag)
            if lag >= 0:
                X[lag:, i, l] = x[:max(T - lag, 0)]
            else:
                X[:max(T + lag, 0), i, l] = x[-lag:]
    return names, lags, X


def quantise_predictors(X, kid, standardize):
    """Listwise deletion and the fixed point: (kid with -1 on every step where a predictor is missing, n_dropped, zq int32
    (T, I * L), means (I, L), scales (I, L)).  With ``standardize`` a predictor is centred and scaled by its mean and
    (population) standard deviation over the used steps; otherwise mean 0 and scale 1."""
    T, I, L = X.shape
    missing = np.isnan(X).any(axis=(1, 2))
    n_dropped = int((missing & (kid >= 0)).sum())
    kid = np.where(missing, -1, kid).astype(np.int32)
    used = kid >= 0
    means, scales = np.zeros((I, L)), np.ones((I, L))
    if standardize and used.any():
        means = X[used].mean(axis=0)
        scales = X[used].std(axis=0)
        if (scales == 0.0).any():
            raise XmhwException("an index is constant over the used steps: it cannot be standardised")
    z = np.where(used[:, None, None], (np.where(used[:, None, None], X, 0.0) - means) / scales, 0.0)
    zq = np.rint(z * _ONE)
    if zq.size and np.abs(zq).max() >= _ZLIM:
        raise XmhwException("a predictor lies 2**7 and more from zero" + (" after standardisation" if standardize else
                            ": pass standardize=True, or scale the index yourself"))
    return kid, n_dropped, np.ascontiguousarray(zq.reshape(T, I * L), dtype=np.int32), means, scales


# ---- the device stage --------------------------------------------------------------------------------

class _Accumulators(Accumulators):
    """One call's arguments and its device accumulators (FIELDS) with the range counter."""
    range_texts = {"n_range": _RANGE_TEXT}

    def __init__(self, classes, K, zq):
        super().__init__()
        self.hr = hip_regress()
        self.args = (classes, K, zq)

    def begin(self, T, C):
        """T steps, C ocean cells"""
        self.classes, self.K, self.zq = check_regress_arguments(T, *self.args)
        K, J = self.K, int(self.zq.shape[1])
        self.make(C, {k: ((K, C) if k in _PER_CELL else (K, J, C), np.int32 if k in ("n", "n1") else np.int64)
                      for k in FIELDS})
        with as_xmhw_errors(also="Unsupported"):
            self.hr.index_regress_init(K, J, C, *self.ptrs(), C, self.count.ptr)

    def add_slab(self, slab):
        """One slab (series_stage.Slab), columns k0..k0+n-1 of the accumulators; the base is where the slab carries its
        climatologies."""
        with as_xmhw_errors(also="Unsupported"):
            self.hr.index_regress_accumulate(slab.d_ts.ptr, slab.isz, slab.T, slab.n, slab.ld, slab.se_ptr, slab.ldc, slab.D,
                                             slab.rows, self.classes, self.K, self.zq, *self.ptrs(slab.k0), self.C,
                                             self.count.ptr)
        self.h.stream_sync(0)                           # the slab's series is freed on the way out


def _bytes_per_cell(T, isz, D):
    return T * isz + 2 * D * 8 + 64


def regress_cells(ts, base, doy, doys, classes, K, zq, max_batch_bytes=64 << 30, pad=None, counters=None):
    """The device stage for a dense (T, C) series: base (D, C) with the labels doy (T,) / doys (D,) that pair steps and
    base rows as in detect_front.detect_cells, classes (T,) int labels in [-1, K), zq (T, J) int.  Returns the eight
    arrays of FIELDS.  Cells go through the device in batches below max_batch_bytes; the sums are integers, so the batch
    size does not change a single bit.  Raises if a sample is out of range (module docstring); with ``counters`` (a dict)
    it stores ``n_range`` there instead."""
    return run_cells(_Accumulators(classes, K, zq), ts, base, base, doy, doys, _bytes_per_cell, max_batch_bytes, pad, counters)


def regress_grid(stacked, anynans, base, doy, doys, classes, K, zq, max_batch_bytes=None, clim_stacked=False, pad=None,
                 counters=None):
    """regress_cells() for an UNCOMPACTED stacked host series (T, N), float or a packed int16 view: the land mask and the
    compaction run on the device slab by slab (series_stage.walk_grid).  Returns the eight arrays over the ocean cells
    and keep[N]."""
    out, keep = run_grid(_Accumulators(classes, K, zq), stacked, anynans, base, base, doy, doys,
                         lambda T, D: 4 * D * 8 + 64, max_batch_bytes, clim_stacked, pad, counters)
    return out + (keep,)


# ---- the result --------------------------------------------------------------------------------------

def class_totals(kid, K, zq):
    """What the host computes once per call, as exact integers: per class the used steps N (K,), the sums Z and ZZ (K, J)
    of zq and zq**2 over them, and over the pairs of consecutive steps that are both of the class their number N1 (K,)
    and the sums Z0, Z1, ZZ0, ZZ1 and Z01 (K, J) of zq(t - 1), zq(t), their squares and their product."""
    z = zq.astype(np.int64)
    J = z.shape[1]
    out = {k: np.zeros((K, J), np.int64) for k in ("Z", "ZZ", "Z0", "Z1", "ZZ0", "ZZ1", "Z01")}
    out["N"], out["N1"] = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for k in range(K):
        sel = kid == k
        pair = np.zeros_like(sel)
        pair[1:] = sel[1:] & sel[:-1]
        now, before = z[pair], z[np.roll(pair, -1)]              # pair[0] is never set: the roll wraps nothing
        out["N"][k], out["N1"][k] = sel.sum(), pair.sum()
        out["Z"][k], out["ZZ"][k] = z[sel].sum(axis=0), (z[sel] ** 2).sum(axis=0)
        out["Z0"][k], out["Z1"][k] = before.sum(axis=0), now.sum(axis=0)
        out["ZZ0"][k], out["ZZ1"][k], out["Z01"][k] = (before ** 2).sum(axis=0), (now ** 2).sum(axis=0), (before * now).sum(axis=0)
    return out


class IndexRegressionDataset:
    """What index_regression() returns, as plain arrays.

    klass (K,) the class labels (sorted non-negative labels found), n_steps (K,) the used steps of each class, index (I,)
    the index names, lag (L,) the lags in steps, n_dropped the steps that listwise deletion took out, means / scales
    (I, L) of the standardisation (0 and 1 without it), totals: class_totals() of the call.
    Raw integers on the grid: n, n1 int32 and sa, saa, saa1 int64 over (klass, *spatial dims); saz, mz, mzz int64 over
    (klass, index, lag, *spatial dims).
    Derived float64, computed here from the integers, with sz = Z - mz and szz = ZZ - mzz the cell's own predictor sums,
    Sxy = saz - sa sz / n, Sxx = szz - sz**2 / n, Syy = saa - sa**2 / n:
        mean       (klass, ...)               sa / n / 2**16: the mean anomaly over the valid steps
        slope      (klass, index, lag, ...)   Sxy / Sxx / scale: anomaly per ORIGINAL unit of the index
        intercept  (klass, index, lag, ...)   the anomaly at index = 0: mean - slope * (index mean over the cell's steps)
        r          (klass, index, lag, ...)   Sxy / sqrt(Sxx Syy)
        r1         (klass, ...)               (saa1 / n1 - m**2) / (saa / n - m**2), m = sa / n: the cell's lag-1
                                              autocorrelation within the class
        r1z        (klass, index, lag)        the predictor's own lag-1 autocorrelation over the pairs of consecutive
                                              steps of the class (the Pearson correlation of z(t - 1) and z(t) over them)
        n_eff      (klass, index, lag, ...)   n (1 - r1 r1z) / (1 + r1 r1z) (Bretherton et al. 1999), clipped to [2, n]
        p_value    (klass, index, lag, ...)   two-sided, Student's t with n_eff - 2 degrees of freedom of
                                              r sqrt((n_eff - 2) / (1 - r**2)); NaN where n_eff = 2.  Computed on first use.
    r1z is taken over the pairs of the class, not over the cell's own valid pairs: the deficits carry no pair products,
    so for a cell with missing samples it is the value of the complete series.
    Land: grid lines without an ocean cell are dropped, as in ClassDaysDataset; the float fields are NaN on the remaining
    land cells, integer fields are 0 there and come with the boolean ``keep`` (...) mask of the ocean cells."""

    def __init__(self, klass, n_steps, index, lag, n_dropped, means, scales, totals, raw, keep, sdims, coords, tdim="time",
                 attrs=None):
        self.klass, self.n_steps = np.asarray(klass), np.asarray(n_steps)
        self.index, self.lag, self.n_dropped = tuple(index), np.asarray(lag), int(n_dropped)
        self.means, self.scales, self.totals = np.asarray(means), np.asarray(scales), totals
        for k in FIELDS:
            setattr(self, k, raw[k])
        self.keep, self.sdims, self.coords = keep, tuple(sdims), dict(coords)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        self._p = None
        self._derive()

    def _derive(self):
        K, I, L = self.klass.shape[0], len(self.index), self.lag.shape[0]
        g = self.n.ndim - 1
        cell = lambda a: a.astype(np.float64).reshape((K,) + (1,) * 2 + self.n.shape[1:])          # noqa: E731
        pred = lambda a: a.astype(np.float64).reshape((K, I, L) + (1,) * g)                          # noqa: E731
        n, sa, saa = cell(self.n), cell(self.sa), cell(self.saa)
        sz, szz, saz = pred(self.totals["Z"]) - self.mz, pred(self.totals["ZZ"]) - self.mzz, self.saz.astype(np.float64)
        scale, centre = self.scales.reshape((1, I, L) + (1,) * g), self.means.reshape((1, I, L) + (1,) * g)
        with np.errstate(divide="ignore", invalid="ignore"):
            self._Sxy, self._Sxx, self._Syy = saz - sa * sz / n, szz - sz * sz / n, saa - sa * sa / n
            m = sa / n
            self.mean = (m / _ONE)[:, 0, 0]
            b = self._Sxy / self._Sxx                                # anomaly per standardised unit (both in 2**-16)
            self.slope = b / scale
            self.intercept = (m - b * (sz / n)) / _ONE - self.slope * centre
            self.r = self._Sxy / np.sqrt(self._Sxx * self._Syy)
            n1 = cell(self.n1)
            r1 = (cell(self.saa1) / n1 - m * m) / (saa / n - m * m)
            self.r1 = r1[:, 0, 0]
            t = {k: self.totals[k].astype(np.float64) for k in ("Z0", "Z1", "ZZ0", "ZZ1", "Z01")}
            N1 = self.totals["N1"].astype(np.float64)[:, None]
            self.r1z = ((t["Z01"] - t["Z0"] * t["Z1"] / N1)
                        / np.sqrt((t["ZZ0"] - t["Z0"] ** 2 / N1) * (t["ZZ1"] - t["Z1"] ** 2 / N1))).reshape(K, I, L)
            rr = r1 * self.r1z.reshape((K, I, L) + (1,) * g)
            self.n_eff = np.minimum(np.maximum(n * (1.0 - rr) / (1.0 + rr), 2.0), n * np.ones_like(rr))
        land = ~np.asarray(self.keep, dtype=bool)
        for a in (self.mean, self.slope, self.intercept, self.r, self.r1, self.n_eff):
            a[..., land] = np.nan

    @property
    def p_value(self):
        if self._p is None:
            with np.errstate(divide="ignore", invalid="ignore"):
                dof = self.n_eff - 2.0
                t = self.r * np.sqrt(dof / (1.0 - self.r * self.r))
                self._p = p_two_sided(t, dof)
        return self._p

    def quantisation_bound(self):
        """(slope_bound, r_bound), float64 arrays shaped like ``slope``: how far ``slope`` and ``r`` can lie from the
        least-squares slope and the Pearson correlation of the UNQUANTISED float64 anomalies and (standardised)
        predictors over the same steps.  Derived from the roundings, not fitted.

        Write e = 2**-17.  The stored numbers are q = 2**16 (a + d) and zq = 2**16 (z + f) with |d|, |f| <= e.  For the n
        steps of a cell and class let zc, ac, fc, dc be the centred vectors, sz = |zc| / sqrt(n) and sa = |ac| / sqrt(n)
        the exact standard deviations and sz', sa' those of the stored numbers.  Centring does not lengthen a vector, so
        |fc|, |dc| <= sqrt(n) e, and by the triangle inequality sz <= sz' + e, sz >= sz' - e, sa <= sa' + e.
          Sxy' - Sxy = <zc, dc> + <fc, ac> + <fc, dc>,  so |Sxy' - Sxy| <= n e (sz + sa + e);
          Sxx' - Sxx = 2 <zc, fc> + |fc|**2,            so |Sxx' - Sxx| <= n e (2 sz + e).
        slope: b' - b = ((Sxy' - Sxy) - b (Sxx' - Sxx)) / Sxx' with |b| = |r| sa / sz <= sa / sz and Sxx' = n sz'**2:
          |b' - b| <= e ((sz + sa + e) + (sa / sz) (2 sz + e)) / sz'**2
        evaluated with the upper ends sz' + e, sa' + e and the lower end sz' - e in the quotient (infinite where
        sz' <= e), then divided by the scale of the standardisation like the slope itself.
        r: r = <u, w> for the unit vectors u = zc / |zc|, w = ac / |ac|.  |x / |x| - y / |y|| <= 2 |x - y| / |x| for
        any two vectors, so |u' - u| <= 2 e / sz' and |w' - w| <= 2 e / sa', and
          |r' - r| <= |u' - u| + |w' - w| <= 2 e (1 / sz' + 1 / sa').
        The float64 evaluation from the integers: the integers convert with a relative error of 2**-53, and
        Sxy = saz - sa sz / n takes three more roundings of terms no larger than |saz| + |sa sz| / n, so its absolute
        error is below 2**-50 (|saz| + |sa sz| / n) =: gxy, likewise gxx and gyy; they move b by (gxy + |b| gxx) / Sxx and
        r by gxy / sqrt(Sxx Syy) + |r| (gxx / Sxx + gyy / Syy) / 2, and the final quotient and root add 2**-50 relative.
        Both are added.  They stay small while the mean of a series is no larger than its standard deviation; a series
        far from zero in units of its spread loses digits in Sxx and Syy, and the bound says so."""
        e = 2.0 ** -17
        K, I, L = self.klass.shape[0], len(self.index), self.lag.shape[0]
        g = self.n.ndim - 1
        f64 = lambda a, shape: np.abs(a.astype(np.float64)).reshape(shape)                           # noqa: E731
        cshape, pshape = (K, 1, 1) + self.n.shape[1:], (K, I, L) + (1,) * g
        n, sa, saa = f64(self.n, cshape), f64(self.sa, cshape), f64(self.saa, cshape)
        sz = np.abs(self.totals["Z"].astype(np.float64).reshape(pshape) - self.mz)
        szz = np.abs(self.totals["ZZ"].astype(np.float64).reshape(pshape) - self.mzz)
        with np.errstate(divide="ignore", invalid="ignore"):
            sdz, sda = np.sqrt(self._Sxx / n) / _ONE, np.sqrt(self._Syy / n) / _ONE
            hi_z, hi_a, lo_z = sdz + e, sda + e, np.where(sdz > e, sdz - e, 0.0)
            b = np.abs(self._Sxy / self._Sxx)
            slope = e * ((hi_z + hi_a + e) + (hi_a / lo_z) * (2.0 * hi_z + e)) / (sdz * sdz)
            r = 2.0 * e * (1.0 / sdz + 1.0 / sda)
            u = 2.0 ** -50
            gxy, gxx, gyy = u * (np.abs(self.saz) + sa * sz / n), u * (szz + sz * sz / n), u * (saa + sa * sa / n)
            slope = slope + (gxy + b * gxx) / self._Sxx + u * b
            r = r + gxy / np.sqrt(self._Sxx * self._Syy) + np.abs(self.r) * (gxx / self._Sxx + gyy / self._Syy) / 2.0 + u
            slope = slope / self.scales.reshape((1, I, L) + (1,) * g)
        bad = ~(self._Sxx > 0.0) | ~(self._Syy > 0.0) | ~(lo_z > 0.0)
        return np.where(bad, np.inf, slope), np.where(bad, np.inf, r)

    def to_xarray(self):
        import xarray as xr
        cell, pred = ("klass",) + self.sdims, ("klass", "index", "lag") + self.sdims
        data = {k: (cell if getattr(self, k).ndim == len(cell) else pred, getattr(self, k)) for k in FIELDS}
        data.update({k: (pred, getattr(self, k)) for k in ("slope", "intercept", "r", "n_eff", "p_value")})
        data.update(mean=(cell, self.mean), r1=(cell, self.r1), r1z=(("klass", "index", "lag"), self.r1z),
                    n_steps=(("klass",), self.n_steps), keep=(self.sdims, self.keep),
                    index_mean=(("index", "lag"), self.means), index_scale=(("index", "lag"), self.scales))
        return xr.Dataset(data, coords=dict({"klass": self.klass, "index": list(self.index), "lag": self.lag},
                                            **{d: self.coords[d] for d in self.sdims}),
                          attrs=dict(self.attrs, n_dropped=self.n_dropped))


# ---- the public function -----------------------------------------------------------------------------

def index_regression(temp, base, indices, lags=(0,), classes="all", standardize=True, tdim="time", maxPadLength=None,
                     tstep=False, anynans=False, max_batch_bytes=None, _compute=None):
    """Lagged regression maps: per cell and class of time steps, the regression and correlation of the anomaly
    ``temp - base`` on every index of ``indices`` at every lag of ``lags``.

    ``temp``, ``base`` and the shared options mean and validate what they do in heat_stress(): land masking, padding, a
    constant base per cell or a ('doy', ...) climatology such as ``seas`` of threshold().  ``indices``: a dict from name
    to a series of length T, NaN = missing; a one-region ``region_series().series()`` is taken as it is.  ``lags``:
    whole numbers of steps, positive = the index leads: predictor (i, l) is x_i(t - lags[l]); at most 32 predictors.  A
    step on which any predictor is missing or falls off the time axis counts nowhere (listwise deletion: all lags share
    one sample) and is counted in ``n_dropped``.  ``classes``: as in mhw_days_by(), at most 64.  ``standardize``: centre
    and scale every predictor over the used steps before the fixed point (the slopes are reported per original unit
    either way); without it a predictor must lie inside (-2**7, 2**7) as it is.

    Returns an IndexRegressionDataset.  Raises if a sample lies 2**7 and more from its base.  ``_compute``: a stand-in
    for regress_cells() (host tests)."""
    layout = grid_layout(temp, tdim)
    coords, _, _, point, sdims, sshape, N = layout
    time = np.asarray(coords[tdim])
    T = time.shape[0]
    check_steps(T, "index_regression")
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "index_regression", "classes")
    names, lags, X = lagged_predictors(indices, lags, T)
    kid, n_dropped, zq, means, scales = quantise_predictors(X, kid, bool(standardize))
    kid, K, zq = check_regress_arguments(T, kid, K, zq)
    base = base_series(base, point, sdims, coords)
    I, L, J = len(names), lags.shape[0], zq.shape[1]
    f, arrays, mhw = cell_stage(
        "regression", temp, base, base, layout, tdim,
        lambda host_keep, ts, sec, thc, doy, doys, options, **extra:
            (_compute or regress_cells)(ts, sec, doy, doys, kid, K, zq, **extra),
        lambda stacked, anynans_, sec, thc, doy, doys, options, **extra:
            regress_grid(stacked, anynans_, sec, doy, doys, kid, K, zq, **extra),
        lambda C: [(K, C)] * 5 + [(K, J, C)] * 3, _Accumulators.range_texts, maxPadLength=maxPadLength, tstep=tstep,
        anynans=anynans, _compute=_compute, max_batch_bytes=max_batch_bytes)
    raw = {}
    for k, a in zip(FIELDS, arrays):
        a = a.reshape((K, I, L, f.C)) if a.ndim == 3 else a
        raw[k] = f.place(a, 0, np.int32 if k in ("n", "n1") else np.int64)
    totals = class_totals(kid, K, zq)
    attrs = stage_attrs(classes, mhw, standardize=bool(standardize))
    return IndexRegressionDataset(class_result_labels(found), totals["N"], names, lags, n_dropped, means, scales, totals, raw,
                                  f.keep, f.sdims, f.coords, tdim, attrs)
