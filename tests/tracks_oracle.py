"""mhw_tracks() restated by brute force: the definition the device is compared with.

* tracks_dense(): every selected object's rows are rasterised into a dense (duration, ny, nx) boolean block and the
  cells of each day are summed one by one with Python integers; weights, unit vectors and centres are computed here
  with ``math`` from the coordinates, nothing is taken from xmhw_amd.tracks.  On purpose it knows nothing of
  difference arrays or prefix sums.
* stage_voxels(): the stage contract of xmhw_amd.tracks.tracks_device on compact arrays, by expanding every row into
  its days and adding them one at a time (numpy's add.at) -- the stand-in for the device in the host tests and the
  reference of the large synthetic GPU cases.
"""
import math

import numpy as np

LAT = ("lat", "latitude", "y", "yt_ocean", "nav_lat")
LON = ("lon", "longitude", "x", "xt_ocean", "nav_lon")
COL_START, COL_END = 1, 2                                        # index_start, index_end of EventDataset.columns


def stage_voxels(start, end, slot, cell, vec, time_start, offsets):
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    slot, cell = np.asarray(slot, dtype=np.int64), np.asarray(cell, dtype=np.int64)
    vec, offsets = np.asarray(vec, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    m = offsets.shape[0] - 1
    L = int(offsets[-1])
    rows = np.nonzero((slot >= 0) & (slot < m))[0]
    d = end[rows] - start[rows] + 1
    r = np.repeat(rows, d)
    day = np.arange(int(d.sum()), dtype=np.int64) - np.repeat(np.cumsum(d) - d, d) + start[r]
    k = offsets[slot[r]] + day - np.asarray(time_start, dtype=np.int64)[slot[r]]
    assert k.size == 0 or (k.min() >= 0 and (k < offsets[slot[r] + 1]).all())
    n_cells = np.zeros(L, dtype=np.int64)
    np.add.at(n_cells, k, 1)
    sums = np.zeros((4, L), dtype=np.int64)
    for c in range(4):
        np.add.at(sums[c], k, vec[c, cell[r]])
    return dict(n_cells=n_cells.astype(np.int32), sums=sums)


def _names(ds):
    lat = [d for d in ds.sdims if d.lower() in LAT and d in ds.coords]
    lon = [d for d in ds.sdims if d.lower() in LON and d in ds.coords]
    return (lat[0], lon[0]) if len(lat) == 1 and len(lon) == 1 else None


def grid_weights(ds, weights):
    """(N,) float64 in stacked order"""
    ny, nx = ds.sshape
    if weights is None:
        return np.ones(ny * nx)
    if isinstance(weights, str):
        k = [d.lower() in LAT for d in ds.sdims].index(True)
        c = np.cos(np.deg2rad(np.asarray(ds.coords[ds.sdims[k]], dtype=np.float64)))
        c = np.where(np.abs(c) < 1e-15, 0.0, c)
        return (np.repeat(c, nx) if k == 0 else np.tile(c, ny)).astype(np.float64)
    return np.asarray(weights, dtype=np.float64).reshape(-1)


def tracks_dense(ds, obj, ids=None, weights=None):
    """dict of flat lists / arrays in CSR order: offsets, n_cells, area_q, mx, my, mz, wsum, lat, lon (from the
    integers), flat, flon (the centre of the unquantised float64 weights), ci, cj (index mode), mode, mb"""
    ny, nx = (int(v) for v in ds.sshape)
    ids = list(range(obj.n_objects)) if ids is None else [int(i) for i in ids]
    w = grid_weights(ds, weights)
    C = int(ds.n_cells)
    names = _names(ds)
    bits = int(obj.weight_bits)
    ubits = 20 if names else max(ny, nx).bit_length()
    mb = min(bits, 61 - ubits - C.bit_length())
    wmax = float(w.max())
    wq = [int(v) for v in np.rint(w / wmax * 2 ** bits)]
    wm = [int(v) for v in np.rint(w / wmax * 2 ** mb)]
    if names:
        k_lat = ds.sdims.index(names[0])
        lat = [math.radians(float(v)) for v in ds.coords[names[0]]]
        lon = [math.radians(float(v)) for v in ds.coords[names[1]]]
        lon_min = min(float(v) for v in ds.coords[names[1]])
        lon0 = -180.0 if lon_min < 0 else 0.0
        e, u = [], []
        for p in range(ny * nx):
            i, j = divmod(p, nx)
            la, lo = (lat[i], lon[j]) if k_lat == 0 else (lat[j], lon[i])
            v = (math.cos(la) * math.cos(lo), math.cos(la) * math.sin(lo), math.sin(la))
            e.append(v)
            u.append(tuple(int(np.rint(2.0 ** 20 * t)) for t in v))
    flat_of_row = np.asarray(ds.cell_index)[np.repeat(np.arange(C), np.diff(ds.offsets))]
    start = ds.table[:, COL_START].astype(np.int64)
    end = ds.table[:, COL_END].astype(np.int64)
    out = {k: [] for k in ("n_cells", "area_q", "mx", "my", "mz", "wsum", "lat", "lon", "flat", "flon", "ci", "cj")}
    offsets = [0]
    for o in ids:
        t0, t1 = int(obj.time_start[o]), int(obj.time_end[o])
        block = np.zeros((t1 - t0 + 1, ny, nx), dtype=bool)
        for r in np.nonzero(np.asarray(obj.object) == o)[0]:
            i, j = divmod(int(flat_of_row[r]), nx)
            assert not block[start[r] - t0:end[r] + 1 - t0, i, j].any()
            block[start[r] - t0:end[r] + 1 - t0, i, j] = True
        offsets.append(offsets[-1] + block.shape[0])
        for day in block:
            cells = [int(p) for p in np.nonzero(day.reshape(-1))[0]]
            out["n_cells"].append(len(cells))
            out["area_q"].append(sum(wq[p] for p in cells))
            out["wsum"].append(sum(wm[p] for p in cells))
            if names:
                M = [sum(wm[p] * u[p][a] for p in cells) for a in range(3)]
                F = [math.fsum(w[p] * e[p][a] for p in cells) for a in range(3)]
                for key, vx, vy, vz in (("l", *M), ("fl", *F)):
                    if vx == 0 and vy == 0 and vz == 0:
                        la = lo = float("nan")
                    else:
                        la = math.degrees(math.atan2(float(vz), math.hypot(float(vx), float(vy))))
                        lo = math.degrees(math.atan2(float(vy), float(vx)))
                        if lo < lon0:
                            lo += 360.0
                        if lo >= lon0 + 360.0:
                            lo -= 360.0
                    out[key + "at"].append(la)
                    out[key + "on"].append(lo)
            else:
                M = [sum(wm[p] * (p // nx) for p in cells), sum(wm[p] * (p % nx) for p in cells), 0]
                ws = out["wsum"][-1]
                out["ci"].append(M[0] / ws if ws else float("nan"))
                out["cj"].append(M[1] / ws if ws else float("nan"))
                fw = math.fsum(w[p] for p in cells)
                out["flat"].append(math.fsum(w[p] * (p // nx) for p in cells) / fw if fw else float("nan"))
                out["flon"].append(math.fsum(w[p] * (p % nx) for p in cells) / fw if fw else float("nan"))
            for a, key in enumerate(("mx", "my", "mz")):
                out[key].append(M[a])
    out.update(offsets=offsets, mode="sphere" if names else "index", mb=mb, ids=ids)
    return out


def arc_degrees(lat1, lon1, lat2, lon2):
    """great-circle distance in degrees between two points given in degrees"""
    a = [math.radians(float(v)) for v in (lat1, lon1, lat2, lon2)]
    p = (math.cos(a[0]) * math.cos(a[1]), math.cos(a[0]) * math.sin(a[1]), math.sin(a[0]))
    q = (math.cos(a[2]) * math.cos(a[3]), math.cos(a[2]) * math.sin(a[3]), math.sin(a[2]))
    cr = (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])
    return math.degrees(math.atan2(math.sqrt(sum(c * c for c in cr)), sum(x * y for x, y in zip(p, q))))


def same_as_dense(tr, want, lonlat_tol=1e-9):
    """every integer equal; the centres within lonlat_tol degrees; the unquantised centre within quantisation_bound()"""
    import numpy.testing as npt
    npt.assert_array_equal(tr.offsets, np.asarray(want["offsets"], dtype=np.int64))
    assert tr.mode == want["mode"] and tr.moment_bits == want["mb"]
    assert tr.n_cells.dtype == np.int32
    for k in ("n_cells", "area_q", "mx", "my", "mz"):
        npt.assert_array_equal(getattr(tr, k), np.asarray(want[k], dtype=np.int64), err_msg=k)
    bound = tr.quantisation_bound()
    if tr.mode == "sphere":
        assert tr.wsum is None
        for k in ("lat", "lon"):
            got, ref = getattr(tr, k), np.asarray(want[k], dtype=np.float64)
            npt.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=k)
            ok = ~np.isnan(ref)
            assert got[ok].size == 0 or np.abs(got[ok] - ref[ok]).max() <= lonlat_tol, k
        for k in range(len(want["lat"])):
            if not (math.isnan(want["lat"][k]) or math.isnan(want["flat"][k])):
                d = arc_degrees(tr.lat[k], tr.lon[k], want["flat"][k], want["flon"][k])
                assert d <= bound[k] + 1e-12, (k, d, bound[k])
    else:
        npt.assert_array_equal(tr.wsum, np.asarray(want["wsum"], dtype=np.int64))
        for k, f in (("ci", "flat"), ("cj", "flon")):
            npt.assert_array_equal(getattr(tr, k), np.asarray(want[k], dtype=np.float64), err_msg=k)
            ok = ~np.isnan(np.asarray(want[f]))
            assert (np.abs(getattr(tr, k) - np.asarray(want[f]))[ok] <= bound[ok] + 1e-12).all(), k
