"""A numpy oracle of regrid() (include/xmhw_amd.h, "regrid()"; xmhw_amd/regrid.py restates the definition): for the
step t and the destination cell (J, I), over the pairs (r, k) of the row run of J and the column run of I with
w = ay * ax > 0 whose sample x[t, row_first[J] + r, (col_first[I] + k) mod nx] is not NaN:
    xq = rint((float64(x) - x0) * 2**16); a pair with |x - x0| >= 2**7, or infinite, is left out and counted (n_range)
    n += 1, wsum += w, xsum += w * xq            (int64; with ``exact=True`` checked against Python integers)
valid iff n >= 1 and wsum * 65536 >= a * wy[J] * wx[I]; out = x0 + (float64(xsum) / float64(wsum)) / 65536.0 in float64 as
written, rounded once to the sample type, NaN where invalid.  It takes what the C entries take (the tables as host
arrays), so it also stands in for the device stage of regrid() in the host tests.  The sums are taken pair by pair over a
dense expansion of the tables, not separably: the kernel's separable order is checked against it."""
import numpy as np

BITS = 16
RANGE = 128.0
MAX_RUN = 64
MAX_WEIGHT = 4096
MAX_EXTENT = 1 << 18


def check_axis(first, ptr, w, full, n, periodic):
    first, ptr, w, full = (np.asarray(v, dtype=np.int64) for v in (first, ptr, w, full))
    m = first.shape[0]
    assert ptr.shape == (m + 1,) and full.shape == (m,) and ptr[0] == 0 and (np.diff(ptr) >= 0).all() and w.shape[0] >= ptr[-1]
    cnt = np.diff(ptr)
    assert (cnt <= MAX_RUN).all() and (w[:ptr[-1]] >= 0).all() and (w[:ptr[-1]] <= MAX_WEIGHT).all() and (full <= MAX_EXTENT).all()
    for k in range(m):
        assert w[ptr[k]:ptr[k + 1]].sum() <= full[k]
        if cnt[k]:
            assert (0 <= first[k] < n and cnt[k] <= n) if periodic else (0 <= first[k] and first[k] + cnt[k] <= n)
    return first, ptr, w, full, cnt


def dense_axis(first, ptr, w, cnt, n, periodic):
    """(index (m, R), weight (m, R)) with R the longest run (1 at least): entry e of run k, weight 0 past the run"""
    m = first.shape[0]
    R = max(int(cnt.max()) if m else 0, 1)
    e = np.arange(R)[None]
    live = e < cnt[:, None]
    idx = first[:, None] + e
    idx = np.where(live, idx % n if periodic else idx, 0)
    at = np.where(live, ptr[:-1, None] + e, 0)
    wt = np.where(live, w[at] if w.shape[0] else 0, 0)
    return idx, wt


def regrid_oracle(field, ny, nx, rows, cols, periodic, x0, a, exact=False):
    """``field`` (T, >= ny * nx) float32 / float64 (columns past ny * nx are padding); ``rows`` = (row_first, row_ptr, ay,
    wy), ``cols`` = (col_first, col_ptr, ax, wx).  Returns (out (T, my * mx) in the dtype of ``field``, wsum int64, n
    int32, n_range)."""
    field = np.asarray(field)
    T = field.shape[0]
    rf, rp, ay, wy, rc = check_axis(*rows, ny, False)
    cf, cp, ax, wx, cc = check_axis(*cols, nx, bool(periodic))
    assert 0 <= a <= 65536 and np.isfinite(x0)
    my, mx = rf.shape[0], cf.shape[0]
    out = np.full((T, my * mx), np.nan, dtype=field.dtype)
    wsum = np.zeros((T, my * mx), dtype=np.int64)
    n = np.zeros((T, my * mx), dtype=np.int32)
    if T == 0 or my == 0 or mx == 0:
        return out, wsum, n, 0
    jj, wj = dense_axis(rf, rp, ay, rc, ny, False)               # (my, R)
    ii, wi = dense_axis(cf, cp, ax, cc, nx, bool(periodic))      # (mx, K)
    x = field[:, :ny * nx].reshape(T, ny, nx)
    least = int(a) * wy[:, None] * wx[None]                      # (my, mx)
    n_range = 0
    # destination columns in groups by run length, so that a few long runs do not pad every column to 64 entries
    groups = [np.nonzero((cc > lo) & (cc <= hi))[0] for lo, hi in ((-1, 4), (4, 17), (17, MAX_RUN))]
    for J in range(my):
        for sel in (g for g in groups if g.size):
            K = max(int(cc[sel].max()), 1)
            w = wj[J][:, None, None] * wi[sel, :K][None]         # (R, mx', K)
            sl = J * mx + sel
            tb = max(1, int(4e6) // w.size)                          # steps at a time: a few million pairs in memory
            for t0 in range(0, T, tb):
                # (tb, R, mx, K): the samples of the footprints of row J
                xs = x[t0:t0 + tb][:, jj[J]][:, :, ii[sel, :K]].astype(np.float64)
                with np.errstate(invalid="ignore"):
                    d = xs - float(x0)
                    sample = (w > 0)[None] & ~np.isnan(d)
                    in_range = np.abs(d) < RANGE                     # +-inf is out
                    use = sample & in_range
                    xq = np.where(use, np.rint(np.where(use, d, 0.0) * 65536.0), 0.0).astype(np.int64)
                n_range += int((sample & ~in_range).sum())
                wq = np.where(use, w[None], 0)
                ns_ = use.sum(axis=(1, 3), dtype=np.int64)
                ws = wq.sum(axis=(1, 3))
                xsum = (wq * xq).sum(axis=(1, 3))
                if exact:
                    big = (wq.astype(object) * xq.astype(object)).sum(axis=(1, 3))
                    assert (big == xsum.astype(object)).all() and all(abs(int(v)) <= 2 ** 59 for v in big.reshape(-1))
                valid = (ns_ >= 1) & (ws * 65536 >= least[J][sel][None])
                with np.errstate(divide="ignore", invalid="ignore"):
                    mean = float(x0) + (xsum.astype(np.float64) / ws.astype(np.float64)) / 65536.0
                out[t0:t0 + tb, sl] = np.where(valid, mean, np.nan).astype(field.dtype)
                wsum[t0:t0 + tb, sl], n[t0:t0 + tb, sl] = ws, ns_
    return out, wsum, n, n_range


def as_stage(field, ny, nx, my, mx, rows, cols, periodic, x0, a, want=True, **_):
    """the oracle with the signature of xmhw_amd.regrid.regrid_grid(): the ``_compute`` of the host tests"""
    assert len(rows[0]) == my and len(cols[0]) == mx
    out, wsum, n, n_range = regrid_oracle(field, ny, nx, rows, cols, periodic, x0, a)
    return out, (wsum if want else None), (n if want else None), n_range
