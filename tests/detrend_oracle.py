"""The model of xmhw_amd.detrend in numpy, one cell at a time, for the tests: numpy.linalg.lstsq in float64 on the
contributing rows for the coefficients (an independent solver: no normal equations), a plain float64 Cholesky of
G = B'B for the pivot ratio of the failure rule, the other failure rules, and the removal.  Also the stand-ins for
the device stages that the host-logic tests pass to detrend._detrend, and an independent restatement of the design
matrix."""
import numpy as np

PIVOT_LIMIT = 1e-6


def design(days_since_ref, order, harmonics):
    """B[T][P] from the time since t_ref in days: x^k (x in decades of 3652.5 days), 1, cos / sin of the annual
    harmonics (years of 365.25 days)"""
    d = np.asarray(days_since_ref, dtype=np.float64)
    x = d / 3652.5
    phi = d / 365.25
    cols = [x ** k for k in range(1, order + 1)] + [np.ones_like(x)]
    for h in range(1, harmonics + 1):
        cols += [np.cos(2 * np.pi * h * phi), np.sin(2 * np.pi * h * phi)]
    return np.stack(cols, axis=1)


def pivot_ratio(Bc):
    """min_j d_j / G_jj of the Cholesky factorisation of G = Bc'Bc, columns in order (NaN / negative pivots come
    back as they are: the caller compares with the limit)"""
    G = Bc.T @ Bc
    P = G.shape[0]
    L = np.zeros((P, P))
    worst = np.inf
    for j in range(P):
        d = G[j, j] - np.sum(L[j, :j] ** 2)
        ratio = d / G[j, j] if G[j, j] != 0 else np.nan
        if not (ratio > 0):
            return ratio if ratio == ratio else np.nan
        worst = min(worst, ratio)
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, P):
            L[i, j] = (G[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    return worst


def fit_cell(y, B, w, min_valid):
    """(beta[P] or NaN, number of contributing samples, pivot ratio or NaN)"""
    y = np.asarray(y, dtype=np.float64)
    P = B.shape[1]
    use = (np.asarray(w) != 0) & ~np.isnan(y)
    n = int(use.sum())
    nan = np.full(P, np.nan)
    if n < max(int(min_valid), P):
        return nan, n, np.nan
    if np.isinf(y[use]).any():
        return nan, n, np.nan
    ratio = pivot_ratio(B[use])
    if not (ratio > PIVOT_LIMIT):
        return nan, n, ratio
    # columns scaled by exact powers of two to an rms near 1 (x^3 in decades over two years has an rms of 4e-4):
    # the same least-squares problem and the same solver, without the rounding error lstsq owes to the columns'
    # units -- up to 1.8e-11 max|y| in that coefficient against a long-double solve, 2.3e-12 with the scaling
    Bu = B[use]
    scale = 2.0 ** np.round(np.log2(np.sqrt(np.mean(Bu ** 2, axis=0))))
    beta = np.linalg.lstsq(Bu / scale, y[use], rcond=None)[0] / scale
    return beta, n, ratio


def remove_cell(y, B, beta, R):
    """float64 detrended values (the caller rounds to the sample type)"""
    s = np.zeros(B.shape[0])
    for k in range(R):
        s = s + beta[k] * B[:, k]
    return np.asarray(y, dtype=np.float64) - s


def detrend_cells(ts, B, w, R, min_valid):
    """All cells of a dense (T, C) series: (detrended (T, C) in ts' dtype, detrended in float64, coef (P, C),
    n_valid (C,), pivot ratio (C,))"""
    ts = np.asarray(ts)
    T, C = ts.shape
    P = B.shape[1]
    out64 = np.empty((T, C))
    coef = np.empty((P, C))
    nvalid = np.empty(C, dtype=np.int32)
    ratio = np.empty(C)
    for c in range(C):
        beta, n, r = fit_cell(ts[:, c], B, w, min_valid)
        coef[:, c], nvalid[c], ratio[c] = beta, n, r
        out64[:, c] = remove_cell(ts[:, c], B, beta, R)
    return out64.astype(ts.dtype), out64, coef, nvalid, ratio


# ---- stand-ins for the device stages of detrend._detrend ---------------------------------------------------------------
def standin_cells(ts, spec):
    ts = np.ascontiguousarray(ts)
    if ts.dtype.kind != "f" or ts.dtype.itemsize not in (4, 8):
        ts = ts.astype(np.float64)
    out, _, coef, nvalid, _ = detrend_cells(ts, spec.basis, spec.weight, spec.R, spec.min_valid)
    return out, coef, nvalid


def standin_grid(stacked, spec, anynans):
    stacked = np.asarray(stacked)
    if stacked.dtype.kind != "f" or stacked.dtype.itemsize not in (4, 8):
        stacked = stacked.astype(np.float64)
    nan = np.isnan(stacked)
    keep = ~(nan.any(axis=0) if anynans else nan.all(axis=0))
    if not keep.any():
        from xmhw_amd import XmhwException
        raise XmhwException("All points of grid are either land or NaN")
    T, N = stacked.shape
    out = np.full((T, N), np.nan, dtype=stacked.dtype)
    coef = np.full((spec.P, N), np.nan)
    nvalid = np.zeros(N, dtype=np.int32)
    o, c, n = standin_cells(np.ascontiguousarray(stacked[:, keep]), spec)
    out[:, keep], coef[:, keep], nvalid[keep] = o, c, n
    return keep, out, coef, nvalid


# ---- test data ---------------------------------------------------------------------------------------------------------
def sst_like(days, C, rng, dtype=np.float32, trend=None):
    """15 + a seasonal cycle of amplitude 2..10 K + unit noise + a trend per decade (default: -0.5..0.5 per cell)"""
    d = np.asarray(days, dtype=np.float64)[:, None]
    amp = rng.uniform(2, 10, C)
    ph = rng.uniform(0, 365.25, C)
    tr = rng.uniform(-0.5, 0.5, C) if trend is None else np.broadcast_to(trend, (C,))
    x = (d - d.mean()) / 3652.5
    y = 15 + amp * np.sin(2 * np.pi * (d - ph) / 365.25) + rng.normal(size=(d.shape[0], C)) + tr * x
    return y.astype(dtype)
