"""The oracle of mhw_composite(): the definition (xmhw_amd/composite.py, module docstring) as a plain numpy loop over
anchor steps and offsets, vectorised over the cells alone.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

FIELDS = ("n", "s", "ss")
ONE = 65536.0


def composite_sums(ts, base, rows, shift, anchors, classes, K, before, after):
    """ts (T, C) float, base (Dr, C) float64 with rows (T,), anchors (T, C) bool, classes (T,) in [-1, K).  Returns a
    dict: n int32, s and ss int64 over (K, D, C), n_range int."""
    ts = np.asarray(ts)
    T, C = ts.shape
    D = before + after + 1
    n = np.zeros((K, D, C), np.int64)
    s = np.zeros((K, D, C), np.int64)
    ss = np.zeros((K, D, C), np.int64)
    n_range = 0
    scale = 2.0 ** -int(shift)
    anchors = np.asarray(anchors, dtype=bool)
    assert anchors.shape == (T, C)
    for t0 in range(T):
        k = int(classes[t0])
        cols = np.nonzero(anchors[t0])[0]
        if k < 0 or cols.size == 0:
            continue
        for d in range(-before, after + 1):
            t = t0 + d
            if not 0 <= t < T:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                a = (ts[t, cols].astype(np.float64) - base[rows[t], cols]) * scale
                real = ~np.isnan(a)
                inside = real & (np.abs(a) < 128.0)
            n_range += int((real & ~inside).sum())
            q = np.rint(a[inside] * ONE).astype(np.int64)
            i = d + before
            n[k, i, cols[inside]] += 1
            s[k, i, cols[inside]] += q
            ss[k, i, cols[inside]] += q * q
    assert n.max(initial=0) < 2 ** 31
    return {"n": n.astype(np.int32), "s": s, "ss": ss, "n_range": n_range}


def anchors_of_table(view, cells, T):
    """(T, C) bool from an anchor table (start == end, offsets over its cells) and the table cell of every column"""
    out = np.zeros((T, len(cells)), dtype=bool)
    for j, cj in enumerate(cells):
        r = view["start"][int(view["offsets"][cj]):int(view["offsets"][cj + 1])]
        out[r, j] = True
    return out


def composite_cells(ts, base, doy, doys, view, cells, classes, K, before, after, shift, counters=None, **_):
    """the stand-in of the device stage (host tests: _compute=)"""
    ts = np.asarray(ts)
    rows = np.searchsorted(np.asarray(doys), np.asarray(doy))
    r = composite_sums(ts, np.asarray(base, dtype=np.float64), rows, shift, anchors_of_table(view, cells, ts.shape[0]),
                       classes, K, before, after)
    if counters is not None:
        counters["n_range"] = r["n_range"]
    return tuple(r[k] for k in FIELDS)
