"""The definition of mean_trend()'s device stage in numpy float64 (test support; numpy only): the semantics of
xmhw_amd/trend.py restated with exactly their order of operations -- sequential over the blocks, vectorised over
the cells -- so that the device can be compared with it bit for bit.

    trend_oracle(planes, x, tcrit, method) -> (nwhat, nstat, ncol)     the signature of trend.trend_device
"""
import numpy as np

_TOP = np.uint64(0x8000000000000000)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def f64_key(v):
    """order-preserving uint64 keys of float64 (IEEE total order on non-NaN values: -0.0 just below +0.0);
    NaN -> the largest key, so that it sorts last"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    b = v.view(np.uint64)
    k = np.where(b & _TOP != 0, b ^ _ALL, b ^ _TOP)
    return np.where(np.isnan(v), _ALL, k)


def key_f64(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    b = np.where(k & _TOP != 0, k ^ _TOP, k ^ _ALL)
    return b.view(np.float64)


def _median_by_keys(keys, n):
    """(s[(n-1)//2] + s[n//2]) / 2 along axis 0 of the keys sorted in total order; n (ncol,) counts the real
    entries of every column (the others hold the NaN key and sort last); n == 0 -> NaN"""
    s = np.sort(keys, axis=0)
    cols = np.arange(keys.shape[1])
    nn = np.maximum(n, 1)
    a = key_f64(s[(nn - 1) // 2, cols])
    b = key_f64(s[nn // 2, cols])
    with np.errstate(invalid="ignore", over="ignore"):
        med = (a + b) / 2.0
    return np.where(n > 0, med, np.nan)


def ols_oracle(y, x, tcrit):
    """y (nb, ncol), x (nb,), tcrit[k] for k residual degrees of freedom -> mean, trend, dtrend (ncol,)"""
    nb, C = y.shape
    valid = ~np.isnan(y)
    m = valid.sum(axis=0)
    bad = (valid & np.isinf(y)).any(axis=0)
    nan = np.full(C, np.nan)
    with np.errstate(all="ignore"):
        sx = np.zeros(C)
        sy = np.zeros(C)
        for b in range(nb):
            sx = np.where(valid[b], sx + x[b], sx)
            sy = np.where(valid[b], sy + y[b], sy)
        md = m.astype(np.float64)
        xb = sx / md
        yb = sy / md
        sxx = np.zeros(C)
        sxy = np.zeros(C)
        for b in range(nb):
            dx = x[b] - xb
            sxx = np.where(valid[b], sxx + dx * dx, sxx)
            sxy = np.where(valid[b], sxy + dx * (y[b] - yb), sxy)
        trend = sxy / sxx
        mean = yb - trend * xb
        ssr = np.zeros(C)
        for b in range(nb):
            r = y[b] - (mean + trend * x[b])
            ssr = np.where(valid[b], ssr + r * r, ssr)
        s = np.sqrt(ssr / (md - 2.0))
        tc = np.asarray(tcrit, dtype=np.float64)[np.clip(m - 2, 0, max(len(tcrit) - 1, 0))] if len(tcrit) else nan
        dtrend = tc * s / np.sqrt(sxx)
    trend = np.where(m >= 2, trend, np.nan)
    mean = np.where(m >= 2, mean, np.where(m == 1, yb, np.nan))
    dtrend = np.where(m >= 3, dtrend, np.nan)
    out = np.stack([mean, trend, dtrend])
    out[:, bad | (m == 0)] = np.nan
    return out


def theil_sen_oracle(y, x):
    """y (nb, ncol), x (nb,) -> trend, mean, mk_s, mk_var (ncol,)"""
    nb, C = y.shape
    valid = ~np.isnan(y)
    m = valid.sum(axis=0).astype(np.int64)
    bad = (valid & np.isinf(y)).any(axis=0)
    out = np.full((4, C), np.nan)
    if nb == 0:
        return out
    i, j = np.triu_indices(nb, 1)
    with np.errstate(all="ignore"):
        dy = y[j] - y[i]                                   # NaN where either block is missing
        slope = dy / (x[j] - x[i])[:, None]
    n_pairs = m * (m - 1) // 2
    if i.size:
        trend = _median_by_keys(f64_key(slope), n_pairs)
        mk_s = np.nansum(np.sign(dy), axis=0)
    else:
        trend = np.full(C, np.nan)
        mk_s = np.zeros(C)
    ymed = _median_by_keys(f64_key(y), m)
    xmed = _median_by_keys(f64_key(np.where(valid, x[:, None], np.nan)), m)
    with np.errstate(all="ignore"):
        mean = ymed - trend * xmed
    cnt = np.zeros((nb, C), dtype=np.int64)                # c_b
    for b in range(nb):
        cnt += (y == y[b]) & valid[b]
    ties = np.where(valid, (cnt - 1) * (2 * cnt + 5), 0).sum(axis=0)
    mk_var = (m * (m - 1) * (2 * m + 5) - ties).astype(np.float64) / 18.0
    out[0] = np.where(m >= 2, trend, np.nan)
    out[1] = np.where(m >= 2, mean, np.where(m == 1, ymed, np.nan))
    out[2] = np.where(m >= 3, mk_s, np.nan)
    out[3] = np.where(m >= 3, mk_var, np.nan)
    out[:, bad | (m == 0)] = np.nan
    return out


def trend_oracle(planes, x, tcrit, method, chunk=256):
    planes = np.asarray(planes, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    nstat, nb, C = planes.shape
    nwhat = 3 if method == "ols" else 4
    out = np.full((nwhat, nstat, C), np.nan)
    for s in range(nstat):
        for c0 in range(0, C, chunk):
            y = planes[s, :, c0:c0 + chunk]
            out[:, s, c0:c0 + chunk] = ols_oracle(y, x, tcrit) if method == "ols" else theil_sen_oracle(y, x)
    return out
