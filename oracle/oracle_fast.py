"""Vectorised CPU oracle for larger parity runs.  TEST INFRASTRUCTURE ONLY.

Same semantics as ``xmhw_oracle.threshold_cells`` (the dumb per-cell
restatement of xmhw/xmhw.py:184-197, 250-307 and identify.py:137-270) but
batched over cells so that a few thousand cells finish in seconds.  It is
checked against the dumb oracle in ``tests/test_oracle_fast.py``; the dumb
oracle in turn is pinned to the reference's fixtures.

Arithmetic: the pooled quantile follows numpy's ``method="linear"`` exactly
(``numpy/lib/_function_base_impl.py`` ``_quantile``/``_lerp``, numpy 2.2.6):
``vi=(n-1)q; lo=floor(vi); g=vi-lo; r=a+(b-a)g; if g>=0.5: r=b-(b-a)(1-g)``.
The pooled mean is sum/n in float64 (numpy's pairwise ``mean`` differs in the
last bits only).
"""
import math

import numpy as np

from xmhw_oracle import XmhwException, runavg, feb29


def pool_index(doy, w):
    """For each distinct doy (ascending) the time indices of its pool
    {t+k : doy[t]==d, |k|<=w, 0<=t+k<T} (identify.py:204-208), with repeats."""
    doy = np.asarray(doy, dtype=np.int64)
    T = doy.shape[0]
    doys = np.unique(doy)
    pools = []
    for d in doys:
        centres = np.nonzero(doy == d)[0]
        idx = (centres[:, None] + np.arange(-w, w + 1)[None, :]).ravel()
        pools.append(idx[(idx >= 0) & (idx < T)])
    return doys, pools


def raw_clim(ts, doy, q, w):
    """Unsmoothed pooled quantile + mean for all cells: (doys, th[D,C], se[D,C])."""
    ts = np.asarray(ts, dtype=np.float64)
    doys, pools = pool_index(doy, w)
    D, C = doys.shape[0], ts.shape[1]
    th = np.full((D, C), np.nan)
    se = np.full((D, C), np.nan)
    cols = np.arange(C)
    for i, idx in enumerate(pools):
        p = np.sort(ts[idx, :], axis=0)             # NaN sorts last
        n = np.sum(~np.isnan(p), axis=0)
        ok = n > 0
        nn = np.where(ok, n, 1)
        vi = (nn - 1) * q
        lo = np.floor(vi).astype(np.int64)
        g = vi - lo
        hi = np.minimum(lo + 1, nn - 1)
        a = p[lo, cols]
        b = p[hi, cols]
        d = b - a
        r = a + d * g
        r2 = b - d * (1 - g)
        r = np.where(g >= 0.5, r2, r)
        th[i] = np.where(ok, r, np.nan)
        s = np.nansum(p, axis=0)
        se[i] = np.where(ok, s / nn, np.nan)
    return doys, th, se


def finish_cell(doys, col, tstep, smooth, width):
    """Feb-29 fix + runavg on the groups PRESENT for one cell (positional)."""
    present = ~np.isnan(col)
    d_c = doys[present]
    v = col[present]
    if v.size and tstep is False:
        v = np.where(d_c != 60, v, feb29(v, d_c))
    if smooth and v.size:
        v = runavg(v, width)
    out = np.full(col.shape, np.nan)
    out[present] = v
    return out


def _exact_sums(win, dyadic):
    """Per row of ``win`` (n, k): the correctly rounded sum (math.fsum), or numpy's for ``dyadic`` data (every
    partial sum exact in float64); a row that holds +-inf gives numpy's result: +-inf, NaN for both signs."""
    if dyadic:
        return np.sum(win, axis=1)
    out = np.empty(win.shape[0])
    pinf = np.isposinf(win).any(axis=1)
    ninf = np.isneginf(win).any(axis=1)
    nan = np.isnan(win).any(axis=1)
    for i, r in enumerate(win.tolist()):
        if nan[i] or (pinf[i] and ninf[i]):
            out[i] = np.nan
        elif pinf[i]:
            out[i] = np.inf
        elif ninf[i]:
            out[i] = -np.inf
        else:
            out[i] = math.fsum(r)
    return out


def finish_exact(doys, col, feb29_fix, smooth, width, dyadic=False):
    """finish_cell's Feb-29 fix + runavg on the groups PRESENT for one cell (positional: rows 59/60/61 are the
    present groups of those doys, the window wraps over the present rows with np.pad(mode="wrap"), so a width
    larger than their number repeats rows), with every 3-point and window sum correctly rounded (math.fsum): each
    output is the float64 nearest to the exact sum, divided once.  ``dyadic``: the data are k/64 values whose sums
    are all exact in float64 -- numpy sums, same result, no fsum loop.

    Returns (out, M): ``out`` as finish_cell, NaN at absent rows; ``M[d]`` the largest sum(|v|)/width (finite v;
    for the Feb-29 row the mean |v| of its 3-point operands) over the window of row d and the ``width - 1`` windows
    before it, counted positionally and circularly -- the scale of what a sliding window sum re-summed every
    ``width`` rows can lose.  Without smoothing M is that Feb-29 magnitude at the Feb-29 row and 0 elsewhere (the
    only arithmetic is the 3-point mean); NaN at absent rows."""
    col = np.asarray(col, dtype=np.float64)
    doys = np.asarray(doys)
    present = ~np.isnan(col)
    d_c = doys[present]
    v = col[present].copy()
    out = np.full(col.shape, np.nan)
    M = np.full(col.shape, np.nan)
    if v.size == 0:
        return out, M
    # magnitude of each operand: |v|, for the Feb-29 row the mean |v| of its 3-point operands (finite ones)
    mag = np.where(np.isfinite(v), np.abs(v), 0.0)
    if feb29_fix and (d_c == 60).any():
        sel = v[np.isin(d_c, [59, 60, 61])]
        v[d_c == 60] = _exact_sums(sel[None, :], dyadic)[0] / sel.size
        mag[d_c == 60] = math.fsum(np.where(np.isfinite(sel), np.abs(sel), 0.0).tolist()) / sel.size
    if not smooth:
        out[present] = v
        M[present] = np.where(d_c == 60, mag, 0.0) if feb29_fix else 0.0
        return out, M
    if width % 2 == 0 or width <= 0:
        raise XmhwException("Running average window should be odd")
    h = (width - 1) // 2
    padded = np.pad(v, h, mode="wrap")
    win = np.lib.stride_tricks.sliding_window_view(padded, width)        # (n, width): the window of each present row
    out[present] = _exact_sums(win, dyadic) / width
    a = np.lib.stride_tricks.sliding_window_view(np.pad(mag, h, mode="wrap"), width).sum(axis=1) / width
    n = v.size
    if width >= n:                                                        # every window is among the width before
        M[present] = a.max()
    else:
        back = (np.arange(n)[:, None] - np.arange(width)[None, :]) % n    # the window of row j and the width-1 before
        M[present] = a[back].max(axis=1)
    return out, M


def dyadic_feb29(doys, a):
    """Make dyadic (k/64) columns of a (D, C) array keep every finish sum exact through the Feb-29 fix: row 60 moves by
    less than its 3-point count times 1/64, in place, so that the sum of the present (non-NaN) rows of doys 59/60/61
    is a multiple of that count -- their mean is then k/64 as well.  Columns where one of them is +-inf stay as they
    are (the mean is +-inf or NaN either way)."""
    doys = np.asarray(doys)
    if not (doys == 60).any():
        return a
    rows = [int(np.nonzero(doys == d)[0][0]) for d in (59, 60, 61) if (doys == d).any()]
    i60 = int(np.nonzero(doys == 60)[0][0])
    three = a[rows]
    pres = ~np.isnan(three)
    k = np.rint(np.where(pres & np.isfinite(three), three, 0.0) * 64).astype(np.int64).sum(axis=0)
    m = pres.sum(axis=0)
    ok = ~np.isnan(a[i60]) & np.isfinite(np.where(pres, three, 0.0)).all(axis=0)
    a[i60] = np.where(ok, a[i60] + ((-k) % np.maximum(m, 1)) / 64.0, a[i60])
    return a


def threshold_cells_fast(ts, doy, pctile=90, windowHalfWidth=5, smoothPercentile=True,
                         smoothPercentileWidth=31, tstep=False, skipna=False,
                         coldSpells=False):
    if smoothPercentileWidth % 2 == 0:
        raise XmhwException("smoothPercentileWidth should be odd")
    ts = np.asarray(ts, dtype=np.float64)
    if ts.ndim == 1:
        ts = ts[:, None]
    if coldSpells:
        ts = -1.0 * ts
    doys, th, se = raw_clim(ts, doy, pctile / 100.0, windowHalfWidth)
    D, C = th.shape
    full = ~np.isnan(th).any(axis=0)
    # cells with every group present: vectorised finish
    if full.any():
        for arr in (th, se):
            v = arr[:, full]
            if tstep is False and (doys == 60).any():
                sel = np.isin(doys, [59, 60, 61])
                v[doys == 60] = np.mean(v[sel], axis=0)
            if smoothPercentile:
                h = (smoothPercentileWidth - 1) // 2
                padded = np.pad(v, ((h, h), (0, 0)), mode="wrap")
                out = np.empty_like(v)
                for i in range(D):
                    out[i] = np.mean(padded[i:i + smoothPercentileWidth], axis=0)
                v = out
            arr[:, full] = v
    for c in np.nonzero(~full)[0]:
        th[:, c] = finish_cell(doys, th[:, c], tstep, smoothPercentile, smoothPercentileWidth)
        se[:, c] = finish_cell(doys, se[:, c], tstep, smoothPercentile, smoothPercentileWidth)
    return doys, th, se


def packed_mean_f64(codes, doy, w, scale, offset, fill=None, negate=False):
    """The pooled mean xmhw_clim_raw_i16 documents for int16 codes with float64 packing attributes
    (xmhw_amd/csrc/packed_src.h): the exact integer sum S of a pool's valid codes, divided once by their
    count n, decoded in float64 with two roundings -- ``(S / n) * scale + offset``, negated for cold spells;
    NaN where a pool has no valid code.  ``fill``: the fill code (None: every code is a value)."""
    codes = np.asarray(codes)
    valid = np.ones(codes.shape, dtype=bool) if fill is None else codes != fill
    c = np.where(valid, codes.astype(np.int64), 0)
    doys, pools = pool_index(doy, w)
    out = np.full((doys.shape[0], codes.shape[1]), np.nan)
    for i, idx in enumerate(pools):
        S = c[idx].sum(axis=0)                      # int64: exact
        n = valid[idx].sum(axis=0)
        m = S.astype(np.float64) / np.where(n > 0, n, 1)
        y = m * scale
        y = y + offset
        out[i] = np.where(n > 0, -y if negate else y, np.nan)
    return out
