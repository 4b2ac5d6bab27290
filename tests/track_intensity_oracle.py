"""mhw_track_intensity() restated by brute force: the definition the device is compared with.

stage_voxels() follows the stage contract of xmhw_amd.track_intensity.track_intensity_cells on a compact (T, C) series:
every selected table row is expanded into its voxels, the anomaly and the category of every voxel come from the
docstring formulas in numpy float64, and the voxels are then visited ONE BY ONE: sums with Python integers, the maximum
with plain float comparison.  It also sums, with math.fsum, the unquantised w * a and w of every entry when ``w`` (the
float64 weights of the compact cells) is given, for quantisation_bound().  On purpose it knows nothing of slabs, chunks
or atomics.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

INTENSITY_BITS = 16


def rows_of_time(doy, doys):
    doys = np.asarray(doys)
    order = np.argsort(doys, kind="stable")
    r = order[np.searchsorted(doys, np.asarray(doy), sorter=order)]
    assert (doys[r] == np.asarray(doy)).all()
    return r


def voxels(ts, seas, thresh, doy, doys, rows, coldSpells=False):
    """(entry, cell, a, category) of every voxel of a selected row, in table order; category 0 = none of the four"""
    start, end = np.asarray(rows.start, dtype=np.int64), np.asarray(rows.end, dtype=np.int64)
    slot, roff = np.asarray(rows.slot, dtype=np.int64), np.asarray(rows.row_offsets, dtype=np.int64)
    t0, offsets = np.asarray(rows.time_start, dtype=np.int64), np.asarray(rows.offsets, dtype=np.int64)
    m = offsets.shape[0] - 1
    cell_of_row = np.repeat(np.arange(roff.shape[0] - 1, dtype=np.int64), np.diff(roff))
    sel = np.nonzero((slot >= 0) & (slot < m))[0]
    d = end[sel] - start[sel] + 1
    r = np.repeat(sel, d)
    day = np.arange(int(d.sum()), dtype=np.int64) - np.repeat(np.cumsum(d) - d, d) + start[r]
    cell = cell_of_row[r]
    entry = offsets[slot[r]] + day - t0[slot[r]]
    assert entry.size == 0 or (entry.min() >= 0 and (entry < offsets[slot[r] + 1]).all())
    x = np.asarray(ts)[day, cell].astype(np.float64)
    if coldSpells:
        x = -x
    k = rows_of_time(doy, doys)[day]
    se, th = np.asarray(seas, dtype=np.float64)[k, cell], np.asarray(thresh, dtype=np.float64)[k, cell]
    a = x - se
    with np.errstate(divide="ignore", invalid="ignore"):
        cats = np.floor(1.0 + (x - th) / (th - se))
    cat = np.where(cats == 1, 1, np.where(cats == 2, 2, np.where(cats == 3, 3, np.where(cats >= 4, 4, 0))))
    return entry, cell, a, cat


def stage_voxels(ts, seas, thresh, doy, doys, rows, wi, coldSpells=False, w=None, **_):
    L = int(np.asarray(rows.offsets)[-1])
    entry, cell, a, cat = voxels(ts, seas, thresh, doy, doys, rows, coldSpells)
    n_valid, wsum, isum = [0] * L, [0] * L, [0] * L
    imax = [float("nan")] * L
    cats = [[0] * L for _ in range(4)]
    fw, fwa = [[] for _ in range(L)], [[] for _ in range(L)]
    n_range = 0
    wi_l = [int(v) for v in np.asarray(wi)]
    w_l = None if w is None else [float(v) for v in np.asarray(w)]
    for p, c, v, k in zip(entry.tolist(), cell.tolist(), a.tolist(), cat.tolist()):
        if v != v:
            continue
        if not abs(v) < 128.0:
            n_range += 1
            continue
        n_valid[p] += 1
        wsum[p] += wi_l[c]
        isum[p] += wi_l[c] * round(v * 65536.0)                   # round(): to nearest, ties to even, as rint
        if not imax[p] >= v:                                     # NaN-initialised
            imax[p] = v
        if k:
            cats[k - 1][p] += 1
        if w_l is not None:
            fw[p].append(w_l[c])
            fwa[p].append(w_l[c] * v)
    assert all(abs(v) < 1 << 61 for v in isum)
    out = dict(n_valid=np.array(n_valid, dtype=np.int32), wsum_i=np.array(wsum, dtype=np.int64),
               isum_q=np.array(isum, dtype=np.int64), intensity_max=np.array(imax, dtype=np.float64) + 0.0,
               cat_cells=np.array(cats, dtype=np.int32).reshape(4, L), n_range=n_range, n_bad=0)
    if w_l is not None:
        out["mean_unquantised"] = np.array([math.fsum(x) / math.fsum(y) if y and math.fsum(y) > 0 else float("nan")
                                            for x, y in zip(fwa, fw)])
    return out


def same_integers(got, want):
    """every integer and every maximum equal (the sign of a zero maximum too); ``got`` / ``want``: dicts or datasets"""
    import numpy.testing as npt

    def field(x, k):
        return np.asarray(x[k] if isinstance(x, dict) else getattr(x, k))

    for k in ("n_valid", "wsum_i", "isum_q", "intensity_max", "cat_cells"):
        assert field(got, k).dtype == field(want, k).dtype, k
        npt.assert_array_equal(field(got, k), field(want, k), err_msg=k)
    npt.assert_array_equal(np.signbit(field(got, "intensity_max")), np.signbit(field(want, "intensity_max")))
