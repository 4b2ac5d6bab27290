"""The oracle of lag_correlation(): the definition (include/xmhw_amd.h, "lag_correlation()"; xmhw_amd/lag_correlation.py,
module docstring) by brute force per lag -- x[l:] against y[:T - l] -- in numpy, vectorised over the cells alone.  The
fixed point of csrc/stage_reduce.h is restated here once: a value a is valid iff it is not NaN and |a| < 2**7, and enters
as q = rint(a * 2**16).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

FIELDS = ("n", "sx", "sy", "sxx", "syy", "sxy")
SWAPPED = ("n", "sy", "sx", "syy", "sxx", "sxy")
ONE = 65536.0
RANGE = 128.0


def fixed(ts, base, rows, shift):
    """(q int64 (T, C) with 0 where not valid, valid bool (T, C), out of range bool (T, C))"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = (np.asarray(ts).astype(np.float64) - np.asarray(base, dtype=np.float64)[rows]) * 2.0 ** -int(shift)
        real = ~np.isnan(a)
        valid = real & (np.abs(a) < RANGE)
        q = np.where(valid, np.rint(np.where(valid, a, 0.0) * ONE), 0.0).astype(np.int64)
    return q, valid, real & ~valid


def lag_corr_sums(x, y, base_x, base_y, rows, shift_x, shift_y, classes, K, L):
    """x, y (T, C) float, bases (Dr, C) float64 with rows (T,), classes (T,) in [-1, K), lags 0 .. L.  Returns a dict:
    n int32 and sx, sy, sxx, syy, sxy int64 over (K, L + 1, C), n_range (2,) int64."""
    x = np.asarray(x)
    T, C = x.shape
    classes = np.asarray(classes)
    qx, vx, ox = fixed(x, base_x, rows, shift_x)
    qy, vy, oy = fixed(y, base_y, rows, shift_y)
    out = {k: np.zeros((K, L + 1, C), np.int64) for k in FIELDS}
    for l in range(min(L, T - 1) + 1):
        a, va, b, vb = qx[l:], vx[l:], qy[:T - l], vy[:T - l]            # the later step t = l .. T - 1 and its partner
        pair = va & vb
        for k in range(K):
            m = pair & (classes[l:] == k)[:, None]
            out["n"][k, l] = m.sum(axis=0)
            out["sx"][k, l] = np.where(m, a, 0).sum(axis=0)
            out["sy"][k, l] = np.where(m, b, 0).sum(axis=0)
            out["sxx"][k, l] = np.where(m, a * a, 0).sum(axis=0)
            out["syy"][k, l] = np.where(m, b * b, 0).sum(axis=0)
            out["sxy"][k, l] = np.where(m, a * b, 0).sum(axis=0)
    assert out["n"].max(initial=0) < 2 ** 31
    out["n"] = out["n"].astype(np.int32)
    out["n_range"] = np.array([int(ox[classes >= 0].sum()), int(oy.sum())], dtype=np.int64)
    return out


def lag_corr_lags(x, y, base_x, base_y, rows, shift_x, shift_y, classes, K, lo, hi):
    """the six arrays over the lags lo .. hi (K, hi - lo + 1, C) as the public function defines them -- a negative lag -l
    pairs x(t) with y(t + l), the class that of step t + l -- and (n_range of x, of y): every step at which the field can
    enter a pair counts"""
    first = lag_corr_sums(x, y, base_x, base_y, rows, shift_x, shift_y, classes, K, hi)
    n_range = [int(first["n_range"][0]), int(first["n_range"][1])]
    if lo == 0:
        return tuple(first[k] for k in FIELDS), tuple(n_range)
    second = lag_corr_sums(y, x, base_y, base_x, rows, shift_y, shift_x, classes, K, -lo)
    n_range[0] = int(second["n_range"][1])
    return tuple(np.concatenate([second[s][:, -lo:0:-1], first[k]], axis=1) for k, s in zip(FIELDS, SWAPPED)), tuple(n_range)


def lag_corr_cells(x, y, base_x, base_y, doy, doys, classes, K, lo, hi, shift_x=0, shift_y=0, counters=None, **_):
    """the stand-in of the device stage (host tests: _compute=); y None: the autocorrelation of x"""
    x = np.asarray(x)
    rows = np.searchsorted(np.asarray(doys), np.asarray(doy))
    auto = y is None
    if auto:
        y, base_y, shift_y = x, base_x, shift_x
    out, n_range = lag_corr_lags(x, np.asarray(y), base_x, base_y, rows, shift_x, shift_y, classes, K, lo, hi)
    if auto:
        n_range = (n_range[1], 0)
    if counters is not None:
        counters["n_range_x"], counters["n_range_y"] = n_range
    return out
