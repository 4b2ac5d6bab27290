"""A numpy oracle of coarsen() (include/xmhw_amd.h, "coarsen()"; xmhw_amd/coarsen.py restates the definition): the
integer sums in int64 -- with ``exact=True`` checked against Python integers (object dtype), for the cases at the edge of
the 64 bits --, the validity test in integers and the finish in float64 exactly as the definition writes it.  It takes
what the C entries take, so it also stands in for the device stage of coarsen() in the host tests."""
import numpy as np

BITS = 16
RANGE = 128.0
MAX_VOLUME = 4096


def coarsen_oracle(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win, exact=False):
    """``field`` (T, >= ny * nx) float32 / float64 (columns past ny * nx are padding), ``wi`` (ny * nx,) integers,
    ``win`` (S + 1,) boundaries or (S, 2) [start, stop) pairs.  Returns (out (S, ncy * ncx) in the dtype of ``field``,
    wsum int64, n int32, n_range)."""
    field = np.asarray(field)
    T = field.shape[0]
    win = np.asarray(win, dtype=np.int64)
    if win.ndim == 1:                                    # S + 1 boundaries -> (S, 2) [start, stop) pairs
        win = np.stack([win[:-1], win[1:]], axis=1)
    S = win.shape[0]
    assert S == 0 or (win[0, 0] >= 0 and win[-1, 1] <= T and (win[:, 1] > win[:, 0]).all() and (win[1:, 0] >= win[:-1, 1]).all())
    assert fy >= 1 and fx >= 1 and 0 <= ncy <= -(-ny // fy) and 0 <= ncx <= -(-nx // fx) and 0 <= a <= 65536
    assert S == 0 or fy * fx * int((win[:, 1] - win[:, 0]).max()) <= MAX_VOLUME
    # the part of the grid under the coarse grid, padded to whole blocks with points of weight 0 (they are no samples and
    # add nothing to W: a block that hangs over the grid holds its in-grid points only)
    hy, hx = min(ny, ncy * fy), min(nx, ncx * fx)
    x = field[:, :ny * nx].reshape(T, ny, nx)[:, :hy, :hx].astype(np.float64)
    w = np.asarray(wi).reshape(ny, nx)[:hy, :hx].astype(np.int64)
    pad = ((0, ncy * fy - hy), (0, ncx * fx - hx))
    x = np.pad(x, ((0, 0),) + pad, constant_values=np.nan)
    w = np.pad(w, pad, constant_values=0)
    with np.errstate(invalid="ignore"):
        d = x - float(x0)
        sample = (w > 0)[None] & ~np.isnan(d)
        in_range = np.abs(d) < RANGE                     # +-inf is out
        use = sample & in_range
        xq = np.where(use, np.rint(np.where(use, d, 0.0) * 65536.0), 0.0).astype(np.int64)
    wq = np.where(use, w[None], 0)
    blocks = lambda v: v.reshape(v.shape[:-2] + (ncy, fy, ncx, fx))                                    # noqa: E731
    W = blocks(w).sum(axis=(-3, -1))
    out = np.full((S, ncy * ncx), np.nan, dtype=field.dtype)
    wsum = np.zeros((S, ncy * ncx), dtype=np.int64)
    n = np.zeros((S, ncy * ncx), dtype=np.int32)
    n_range = 0
    for s in range(S):
        t0, t1 = int(win[s, 0]), int(win[s, 1])
        n_range += int((sample[t0:t1] & ~in_range[t0:t1]).sum())
        ns_ = blocks(use[t0:t1]).sum(axis=(0, -3, -1), dtype=np.int64)
        ws = blocks(wq[t0:t1]).sum(axis=(0, -3, -1))
        xs = blocks(wq[t0:t1] * xq[t0:t1]).sum(axis=(0, -3, -1))
        if exact:
            big = blocks(wq[t0:t1].astype(object) * xq[t0:t1].astype(object)).sum(axis=(0, -3, -1))
            assert (big == xs.astype(object)).all() and all(abs(int(v)) <= 2 ** 59 for v in big.reshape(-1))
        valid = (ns_ >= 1) & (ws * 65536 >= int(a) * (t1 - t0) * W)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = float(x0) + (xs.astype(np.float64) / ws.astype(np.float64)) / 65536.0
        out[s] = np.where(valid, mean, np.nan).reshape(-1).astype(field.dtype)
        wsum[s], n[s] = ws.reshape(-1), ns_.reshape(-1)
    return out, wsum, n, n_range


def as_stage(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win, want=True, **_):
    """the oracle with the signature of xmhw_amd.coarsen.coarsen_grid(): the ``_compute`` of the host tests"""
    out, wsum, n, n_range = coarsen_oracle(field, ny, nx, fy, fx, ncy, ncx, wi, x0, a, win)
    return out, (wsum if want else None), (n if want else None), n_range
