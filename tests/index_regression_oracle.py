"""Plain-loop oracle of index_regression().  TEST INFRASTRUCTURE ONLY.  One loop over the steps in time order, every sum
kept in Python integers (object arrays: no 64-bit wrap-around can hide), the previous step remembered as it is: no time
blocks, no class runs, no code shared with the product.  The definitions are those of include/xmhw_amd.h and
xmhw_amd/index_regression.py; the derived fields are evaluated from the integers in exact rational arithmetic."""
from fractions import Fraction
import math

import numpy as np

ONE = 65536
FIELDS = ("n", "sa", "saa", "n1", "saa1", "saz", "mz", "mzz")


def _objects(*shape):
    a = np.empty(shape, dtype=object)
    a.fill(0)
    return a


def _as(a, dtype):
    """Python integers -> a numpy array of ``dtype``; a value that does not fit raises OverflowError"""
    info = np.iinfo(dtype)
    flat = [int(v) for v in a.reshape(-1)]
    if flat and (min(flat) < info.min or max(flat) > info.max):
        raise OverflowError(f"a sum does not fit {np.dtype(dtype).name}")
    return np.array(flat, dtype=dtype).reshape(a.shape)


def regress_sums(ts, base, rows, classes, K, zq):
    """The eight arrays of the C ABI and n_range, for a (T, C) series, a (D, C) base with rows (T,), classes (T,) in
    [-1, K) and the predictor table zq (T, J)."""
    ts, base = np.asarray(ts), np.asarray(base, dtype=np.float64)
    rows, classes, zq = np.asarray(rows), np.asarray(classes), np.asarray(zq, dtype=np.int64)
    T, C = ts.shape
    J = zq.shape[1]
    n, sa, saa, n1, saa1 = (_objects(K, C) for _ in range(5))
    saz, mz, mzz = (_objects(K, J, C) for _ in range(3))
    # what a step is, for all steps at once; the sums below are one loop over the steps
    a = ts.astype(np.float64) - base[rows]
    with np.errstate(invalid="ignore"):
        valid_all = ~np.isnan(a) & (np.abs(a) < 128.0)
    q_all = np.rint(np.where(valid_all, a, 0.0) * 65536.0).astype(np.int64)             # |q| <= 2**23: products fit int64
    n_range = int((~np.isnan(a) & ~valid_all)[classes >= 0].sum())
    prev_class, prev_valid, prev_q = -1, np.zeros(C, bool), np.zeros(C, np.int64)
    for t in range(T):
        k = int(classes[t])
        if k < 0:
            prev_class = -1
            continue
        valid, q = valid_all[t], q_all[t]
        z = zq[t]
        n[k] += valid.astype(object)
        sa[k] += q.astype(object)
        saa[k] += (q * q).astype(object)
        pair = valid & prev_valid if prev_class == k else np.zeros(C, bool)
        n1[k] += pair.astype(object)
        saa1[k] += np.where(pair, q * prev_q, 0).astype(object)
        saz[k] += (z[:, None] * q[None, :]).astype(object)
        if not valid.all():
            mz[k] += np.where(valid[None, :], 0, z[:, None]).astype(object)
            mzz[k] += np.where(valid[None, :], 0, (z * z)[:, None]).astype(object)
        prev_class, prev_valid, prev_q = k, valid, q
    out = {"n": _as(n, np.int32), "n1": _as(n1, np.int32), "n_range": n_range}
    for name, a in (("sa", sa), ("saa", saa), ("saa1", saa1), ("saz", saz), ("mz", mz), ("mzz", mzz)):
        out[name] = _as(a, np.int64)
    return out


def regress_cells(ts, base, doy, doys, classes, K, zq, counters=None, **_):
    """the stand-in of the device stage (host tests: _compute=)"""
    r = regress_sums(ts, base, np.searchsorted(np.asarray(doys), np.asarray(doy)), classes, K, zq)
    if counters is not None:
        counters["n_range"] = r["n_range"]
    return tuple(r[k] for k in FIELDS)


def class_totals(classes, k, zq_j):
    """N, Z, ZZ of one class and predictor column over the steps of the class, and over the pairs of consecutive steps of
    the class N1 and the sums of z(t - 1), z(t), their squares and their product: Python integers"""
    steps = [t for t in range(len(classes)) if classes[t] == k]
    z = [int(v) for v in zq_j]
    pairs = [t for t in steps if t >= 1 and classes[t - 1] == k]
    return {"N": len(steps), "Z": sum(z[t] for t in steps), "ZZ": sum(z[t] ** 2 for t in steps), "N1": len(pairs),
            "Z0": sum(z[t - 1] for t in pairs), "Z1": sum(z[t] for t in pairs), "ZZ0": sum(z[t - 1] ** 2 for t in pairs),
            "ZZ1": sum(z[t] ** 2 for t in pairs), "Z01": sum(z[t] * z[t - 1] for t in pairs)}


def _root(x):
    """sqrt of a non-negative Fraction as float64, from the integer roots of numerator and denominator scaled up"""
    if x <= 0:
        return math.nan if x < 0 else 0.0
    s = 1 << 200
    return math.isqrt(x.numerator * s) / math.isqrt(x.denominator * s)


def derived_exact(n, sa, saa, n1, saa1, saz, mz, mzz, tot, mean_x, scale_x):
    """The derived fields of one (class, predictor, cell) from its integers, every step but the last conversion in
    exact rationals.  ``tot``: class_totals() of the predictor; mean_x, scale_x: its standardisation.  Returns floats."""
    n, sa, saa, n1, saa1, saz = (int(v) for v in (n, sa, saa, n1, saa1, saz))
    sz, szz = tot["Z"] - int(mz), tot["ZZ"] - int(mzz)
    F = Fraction
    Sxy, Sxx, Syy = F(saz) - F(sa * sz, n), F(szz) - F(sz * sz, n), F(saa) - F(sa * sa, n)
    m = F(sa, n)
    b = Sxy / Sxx
    scale, centre = F(scale_x), F(mean_x)
    slope = b / scale
    r = (1 if Sxy >= 0 else -1) * _root(Sxy * Sxy / (Sxx * Syy))
    r1 = (F(saa1, n1) - m * m) / (F(saa, n) - m * m)
    N1 = tot["N1"]
    czz = F(tot["Z01"]) - F(tot["Z0"] * tot["Z1"], N1)
    v0, v1 = F(tot["ZZ0"]) - F(tot["Z0"] ** 2, N1), F(tot["ZZ1"]) - F(tot["Z1"] ** 2, N1)
    r1z = (1 if czz >= 0 else -1) * _root(czz * czz / (v0 * v1))
    rr = float(r1) * r1z
    n_eff = min(max(n * (1.0 - rr) / (1.0 + rr), 2.0), float(n))
    return {"mean": float(m / ONE), "slope": float(slope), "intercept": float((m - b * F(sz, n)) / ONE - slope * centre),
            "r": r, "r1": float(r1), "r1z": r1z, "n_eff": n_eff}
