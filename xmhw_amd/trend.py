"""mean_trend(): counterpart of Oliver's marineHeatWaves.meanTrend() (the member of the detect / blockAverage /
rank / meanTrend family that xmhw never ported) on the BlockDataset of block_average() -- the mean and the
linear trend of every block statistic in every grid cell, with a measure of significance.

Two estimators (csrc/kernels_trend.hip).  For one (cell, statistic) series y[0..nb) along ``years``:

    x[b] = years[b] - mean(years)            float64, computed once on the host; every slope is per year
    valid[b] = not isnan(y[b]),  m = number of valid blocks
    a valid y[b] of +-Inf: every output of the item is NaN (as meanTrend);  m == 0: every output NaN

``method="ols"`` -- what meanTrend does: least squares of y on [1, x] over the valid blocks, in closed form and
in this order of float64 operations (sums sequential in block order, no FMA):

    xb = sum(x)/m, yb = sum(y)/m, Sxx = sum((x-xb)^2), Sxy = sum((x-xb)(y-yb))
    trend = Sxy/Sxx,  mean = yb - trend*xb          (the fitted value at the centre of the WHOLE period: x is
                                                     centred on all blocks, not on the valid ones)
    r = y - (mean + trend*x),  s = sqrt(sum(r^2)/(m-2)),  dtrend = tcrit[m-2]*s / sqrt(Sxx)

``tcrit[k]`` is the two-sided Student-t critical value t.isf(alpha/2, k), a host table (student_t_isf below:
regularised incomplete beta and a bracketed Newton iteration; no scipy).  m == 1: mean = y, trend and dtrend
NaN; m == 2: dtrend NaN.  meanTrend returns numpy.linalg.lstsq's minimum-norm answer for m <= 2 (and a
division by zero for dtrend); NaN is deliberate here: one or two points carry no trend estimate worth a map.

``method="theil_sen"`` -- for the tie-ridden, non-Gaussian statistics (ecount, the day counts).  Over the valid
blocks, pairs i < j, N = m(m-1)/2:

    slope_ij = (y_j - y_i)/(x_j - x_i)                 one IEEE float64 division
    trend = (s[(N-1)//2] + s[N//2]) / 2                on the slopes sorted in IEEE total order (-0.0 before
                                                       +0.0): numpy.median's / scipy.stats.theilslopes' value
    mean = median(y_valid) - trend*median(x_valid)     medians by the same rule: the line's value at x = 0
    mk_s = sum_{i<j} sign(y_j - y_i)                   Mann-Kendall S
    mk_var = (m(m-1)(2m+5) - sum_b (c_b-1)(2c_b+5))/18   c_b = #{j valid: y_j == y_b} (-0.0 == 0.0): the
                                                       tie-corrected variance, numerator exact in integers
    mk_z = (S - sign(S))/sqrt(mk_var)                  0 where S == 0, NaN where mk_var == 0 (all values equal)
    p_value = erfc(|mk_z|/sqrt(2))

The device returns trend, mean, mk_s, mk_var; mk_z and p_value are derived here with numpy / math.erfc, so
nothing the device returns depends on a libm.  m < 2: trend NaN, mean = y if m == 1; m < 3: mk_* and p_value
NaN.  ``alpha`` is recorded but unused by this method: Sen's confidence band is not computed.
"""
import math

import numpy as np

from .device import DeviceScope
from .exception import XmhwException
from .stats import BlockDataset
from ._lib import hip

METHODS = ("ols", "theil_sen")
WHAT = {"ols": ("mean", "trend", "dtrend"),
        "theil_sen": ("trend", "mean", "mk_s", "mk_var", "mk_z", "p_value")}
_DEVICE_WHAT = {"ols": ("mean", "trend", "dtrend"), "theil_sen": ("trend", "mean", "mk_s", "mk_var")}
MAX_BLOCKS = 128          # the Theil-Sen kernel's cap on nb (csrc/kernels.h: kTrendMaxBlocks)


# ---- Student-t critical values on the host ---------------------------------------------------------------------------
def _betacf(a, b, x):
    """continued fraction of the incomplete beta function (modified Lentz), converged to float64"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 2000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-16:
            break
    return h


def _betainc(a, b, x):
    """regularised incomplete beta function I_x(a, b)"""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    lbt = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x)
    if x < (a + 1.0) / (a + b + 2.0):
        return math.exp(lbt) * _betacf(a, b, x) / a
    return 1.0 - math.exp(lbt) * _betacf(b, a, 1.0 - x) / b


def _t_sf(t, dof):
    """P(T > t) of Student's t with dof degrees of freedom, t >= 0"""
    t2 = t * t
    # 1 - x = t^2/(dof + t^2) is formed directly, so that neither tail loses digits
    if t2 < dof:
        return 0.5 - 0.5 * _betainc(0.5, 0.5 * dof, t2 / (dof + t2))
    return 0.5 * _betainc(0.5 * dof, 0.5, dof / (dof + t2))


def _t_two_sided(t, dof):
    """the two-sided p-value of one t statistic: NaN without degrees of freedom or for a NaN, 0 for an infinite t"""
    if not (dof > 0.0) or t != t:
        return math.nan
    return 0.0 if math.isinf(t) else min(1.0, 2.0 * _t_sf(abs(t), dof))


def p_two_sided(t, dof):
    """_t_two_sided() over arrays that broadcast: float64"""
    return np.frompyfunc(_t_two_sided, 2, 1)(t, dof).astype(np.float64)


def student_t_isf(q, dof):
    """t with P(T > t) = q for Student's t with ``dof`` degrees of freedom, 0 < q < 0.5: Newton's iteration
    on the survival function kept inside a bracket, until the step is below one part in 1e15."""
    if not (0.0 < q < 0.5) or dof < 1:
        raise ValueError("student_t_isf needs 0 < q < 0.5 and dof >= 1")
    lo, hi = 0.0, 1.0
    while _t_sf(hi, dof) > q:
        lo, hi = hi, hi * 2.0
    lc = math.lgamma(0.5 * (dof + 1.0)) - math.lgamma(0.5 * dof) - 0.5 * math.log(dof * math.pi)
    t = 0.5 * (lo + hi)
    for _ in range(200):
        f = _t_sf(t, dof) - q
        if f > 0.0:
            lo = t
        else:
            hi = t
        pdf = math.exp(lc - 0.5 * (dof + 1.0) * math.log1p(t * t / dof))
        tn = t + f / pdf                       # d sf / dt = -pdf
        if not (lo < tn < hi):
            tn = 0.5 * (lo + hi)
        if abs(tn - t) <= 1e-15 * abs(tn) or hi - lo <= 1e-16 * hi:
            return tn
        t = tn
    return t


def tcrit_table(alpha, nb):
    """tcrit[k] = t.isf(alpha/2, k) for the residual degrees of freedom k = 1 .. nb-2; entry 0 is unused
    (NaN).  Length max(nb - 1, 1)."""
    tab = np.full(max(int(nb) - 1, 1), np.nan)
    for k in range(1, int(nb) - 1):
        tab[k] = student_t_isf(0.5 * alpha, k)
    return tab


def centred_years(years):
    """x[b] = years[b] - mean(years) in float64"""
    y = np.asarray(years, dtype=np.float64)
    return y - y.mean() if y.size else y


# ---- the device stage ------------------------------------------------------------------------------------------------
def trend_device(planes, x, tcrit, method):
    """The device stage on compact arrays: planes (nstat, nb, ncol) float64, the abscissa x (nb,), the
    tcrit table (tcrit_table(); ignored by theil_sen) and the method.  Returns (nwhat, nstat, ncol) in the
    order ("mean", "trend", "dtrend") for "ols", ("trend", "mean", "mk_s", "mk_var") for "theil_sen"."""
    h = hip()
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    nstat, nb, C = planes.shape
    nwhat = len(_DEVICE_WHAT[method])
    out = np.full((nwhat, nstat, C), np.nan)
    if nstat == 0 or C == 0:
        return out
    if method == "theil_sen" and nb > MAX_BLOCKS:
        raise XmhwException(f"mean_trend(method='theil_sen') handles at most {MAX_BLOCKS} blocks, got {nb}")
    with DeviceScope() as s:
        d_in = s.upload(planes)
        d_x = s.upload(np.ascontiguousarray(x, dtype=np.float64))
        d_out = s.alloc(8 * nwhat * nstat * C)
        if method == "ols":
            d_t = s.upload(np.ascontiguousarray(tcrit, dtype=np.float64))
            h.block_trend_ols(d_in.ptr, nstat, nb, C, C, d_x.ptr, d_t.ptr, d_out.ptr, C)
        else:
            h.block_trend_theil_sen(d_in.ptr, nstat, nb, C, C, d_x.ptr, d_out.ptr, C)
        h.stream_sync(0)
        return d_out.to_array((nwhat, nstat, C), np.float64)


def mann_kendall_z(mk_s, mk_var):
    """(mk_z, p_value) of the continuity-corrected Mann-Kendall statistic: mk_z = (S - sign(S))/sqrt(var)
    (0 where S == 0, NaN where var == 0 or S is NaN), p_value = erfc(|mk_z|/sqrt(2))."""
    s = np.asarray(mk_s, dtype=np.float64)
    v = np.asarray(mk_var, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (s - np.sign(s)) / np.sqrt(v)
    z = np.where(v == 0, np.nan, z)
    z = np.where((s == 0) & (v > 0), 0.0, z)
    p = np.full(z.shape, np.nan)
    ok = ~np.isnan(z)
    p[ok] = [math.erfc(abs(a) / math.sqrt(2.0)) for a in z[ok]]
    return z, p


class TrendDataset:
    """What mean_trend() returns: ``tr[what][statistic]`` has dims ``dims`` (the spatial dims of the
    BlockDataset; 0-d for a point); ``attrs`` records alpha, method and the year axis used."""

    def __init__(self, data, dims, coords, attrs):
        self.data, self.dims, self.coords, self.attrs = data, tuple(dims), coords, attrs

    def __getitem__(self, what):
        return self.data[what]

    def keys(self):
        return self.data.keys()

    def to_xarray(self):
        import xarray as xr
        return xr.Dataset({f"{k}_{what}": (self.dims, v) for what, d in self.data.items() for k, v in d.items()},
                          coords={k: (k, v) for k, v in self.coords.items()}, attrs=dict(self.attrs))


def mean_trend(block, alpha=0.05, method="ols", _compute=None):
    """Mean and linear trend of every block statistic, per grid cell.

    ``block``: the BlockDataset returned by block_average(); all its ``data_vars`` are processed.
    ``method="ols"`` (marineHeatWaves.meanTrend): ``mean`` (the fit at the centre of the period), ``trend`` (per
    year) and ``dtrend``, the half-width of the trend's (1 - alpha) confidence interval.
    ``method="theil_sen"``: the Theil-Sen ``trend`` (median of the pairwise slopes), ``mean`` (the median line
    at the centre of the period) and the Mann-Kendall test ``mk_s``, ``mk_var`` (tie-corrected), ``mk_z``
    (continuity-corrected) and two-sided ``p_value``; ``alpha`` is recorded but unused (no Sen confidence band).
    NaN blocks are left out of a series; fewer than two valid blocks give a NaN trend (module docstring).

    Returns a TrendDataset: ``tr["trend"]["duration"]`` has the spatial dims of ``block``.
    """
    if not isinstance(block, BlockDataset):
        raise XmhwException("mean_trend expects the BlockDataset returned by xmhw_amd.block_average()")
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise XmhwException(f"alpha should be a number in (0, 1), got {alpha!r}")
    if not (0.0 < alpha < 1.0):
        raise XmhwException(f"alpha should be in (0, 1), got {alpha}")
    if method not in METHODS:
        raise XmhwException(f"method should be one of {', '.join(METHODS)}, got {method!r}")
    names = list(block.data_vars)
    years = np.asarray(block.coords["years"], dtype=np.float64)
    nb = years.shape[0]
    if method == "theil_sen" and nb > MAX_BLOCKS:
        raise XmhwException(f"mean_trend(method='theil_sen') handles at most {MAX_BLOCKS} blocks, got {nb}")
    if nb > 1 and not np.all(np.diff(years) > 0):
        raise XmhwException("the years of the BlockDataset should be strictly increasing")
    sshape = tuple(np.asarray(block.data_vars[names[0]]).shape[1:]) if names else ()
    ncol = int(np.prod(sshape, dtype=np.int64))
    planes = np.empty((len(names), nb, ncol))
    for i, k in enumerate(names):
        planes[i] = np.asarray(block.data_vars[k], dtype=np.float64).reshape(nb, ncol)
    x = centred_years(years)
    tcrit = tcrit_table(alpha, nb) if method == "ols" else np.full(1, np.nan)
    compute = _compute or trend_device
    res = np.asarray(compute(planes, x, tcrit, method))
    what = list(_DEVICE_WHAT[method])
    if res.shape != (len(what), len(names), ncol):
        raise XmhwException(f"trend stage returned {res.shape}, expected {(len(what), len(names), ncol)}")
    if method == "theil_sen":
        z, p = mann_kendall_z(res[2], res[3])
        res = np.concatenate([res, z[None], p[None]])
        what += ["mk_z", "p_value"]
    data = {w: {k: res[j, i].reshape(sshape) for i, k in enumerate(names)} for j, w in enumerate(what)}
    coords = {d: np.asarray(block.coords[d]) for d in block.dims[1:] if d in block.coords}
    attrs = {"alpha": alpha, "method": method, "years": years.copy(), "year_centre": float(years.mean()) if nb else np.nan,
             "trend_units": "per year"}
    return TrendDataset(data, block.dims[1:], coords, attrs)
