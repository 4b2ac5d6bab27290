"""The oracle of spatial_correlation(): the definition (include/xmhw_amd.h, "spatial_correlation()";
xmhw_amd/spatial_correlation.py, module docstring) on the uncompacted grid, by a plain loop over the offsets with shifted
views -- the rows and columns of the grid that have a partner against the rows and columns of their partners; across a
periodic seam the columns are taken by index, mod nx; nothing is rolled across an edge that does not wrap.  The fixed
point of csrc/stage_reduce.h is restated here once: a value a is valid iff it is not NaN and |a| < 2**7, and enters as
q = rint(a * 2**16).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

FIELDS = ("n", "sx", "sy", "sxx", "syy", "sxy")
ONE = 65536.0
RANGE = 128.0


def fixed(ts, base, rows, shift):
    """(q int64 (T, N) with 0 where not valid, valid bool (T, N), out of range bool (T, N))"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = (np.asarray(ts).astype(np.float64) - np.asarray(base, dtype=np.float64)[rows]) * 2.0 ** -int(shift)
        real = ~np.isnan(a)
        valid = real & (np.abs(a) < RANGE)
        q = np.where(valid, np.rint(np.where(valid, a, 0.0) * ONE), 0.0).astype(np.int64)
    return q, valid, real & ~valid


def partner_views(ny, nx, dj, di, periodic):
    """(rows of the cells, rows of their partners, columns of the cells, columns of their partners) as index arrays: the
    cells (j, i) whose partner (j + dj, i + di) lies in the grid"""
    j = np.arange(ny)
    j = j[(j + dj >= 0) & (j + dj < ny)]
    i = np.arange(nx)
    if periodic:
        ip = (i + di) % nx
    else:
        i = i[(i + di >= 0) & (i + di < nx)]
        ip = i + di
    return j, j + dj, i, ip


def spatial_corr_sums(ts, base, rows, shift, classes, K, offsets, ny, nx, periodic):
    """ts (T, ny * nx) float, base (Dr, ny * nx) float64 with rows (T,), classes (T,) in [-1, K), offsets (D, 2).  Returns
    a dict: n int32 and sx, sy, sxx, syy, sxy int64 over (K, D, ny * nx), n_range int."""
    ts = np.asarray(ts)
    T = ts.shape[0]
    classes = np.asarray(classes)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 2)
    q, valid, out_of_range = fixed(ts, base, rows, shift)
    q, valid = q.reshape(T, ny, nx), valid.reshape(T, ny, nx)
    D = offsets.shape[0]
    out = {k: np.zeros((K, D, ny, nx), np.int64) for k in FIELDS}
    for e, (dj, di) in enumerate(offsets):
        j, jp, i, ip = partner_views(ny, nx, int(dj), int(di), periodic)
        if not j.size or not i.size:
            continue
        a, va = q[:, j][:, :, i], valid[:, j][:, :, i]
        b, vb = q[:, jp][:, :, ip], valid[:, jp][:, :, ip]
        pair = va & vb
        at = np.ix_(j, i)
        for k in range(K):
            m = pair & (classes == k)[:, None, None]
            out["n"][k, e][at] = m.sum(axis=0)
            out["sx"][k, e][at] = np.where(m, a, 0).sum(axis=0)
            out["sy"][k, e][at] = np.where(m, b, 0).sum(axis=0)
            out["sxx"][k, e][at] = np.where(m, a * a, 0).sum(axis=0)
            out["syy"][k, e][at] = np.where(m, b * b, 0).sum(axis=0)
            out["sxy"][k, e][at] = np.where(m, a * b, 0).sum(axis=0)
    assert out["n"].max(initial=0) < 2 ** 31
    out = {k: v.reshape(K, D, ny * nx) for k, v in out.items()}
    out["n"] = out["n"].astype(np.int32)
    out["n_range"] = int(out_of_range[classes >= 0].sum())
    return out


def spatial_corr_point(ts, base, rows, shift, classes, K, offsets, ny, nx, periodic, j, i):
    """the same sums of ONE grid point in Python integers, pair by pair: {field: (K, D) lists}"""
    q, valid, _ = fixed(ts, base, rows, shift)
    out = {k: [[0] * len(offsets) for _ in range(K)] for k in FIELDS}
    for t in range(np.asarray(ts).shape[0]):
        k = int(classes[t])
        if k < 0 or not valid[t, j * nx + i]:
            continue
        x = int(q[t, j * nx + i])
        for e, (dj, di) in enumerate(offsets):
            jp, ip = j + int(dj), i + int(di)
            if periodic:
                ip %= nx
            if not (0 <= jp < ny and 0 <= ip < nx) or not valid[t, jp * nx + ip]:
                continue
            y = int(q[t, jp * nx + ip])
            for name, v in zip(FIELDS, (1, x, y, x * x, y * y, x * y)):
                out[name][k][e] += v
    return out


def spatial_corr_grid(field, base, rows, classes, K, offsets, ny, nx, periodic=False, shift=0, counters=None, **_):
    """the stand-in of the device stage (host tests: _compute=)"""
    out = spatial_corr_sums(field, base, rows, shift, classes, K, offsets, ny, nx, periodic)
    if counters is not None:
        counters["n_range"] = out["n_range"]
    return tuple(out[k] for k in FIELDS)
