"""Plain numpy brute force of mhw_displacement()'s device stage.  TEST INFRASTRUCTURE ONLY.

For every source it takes the minimum of (dist_m, dj, di) over ALL grid points that qualify and lie within reach: it
uses no candidate list and no order.  It calls the per-pair function the table is built from
(xmhw_amd.displacement.pair_metrics), so equality with the device is exact.  Only the geometry of the DisplacementTable
is read (lat, nx, dlon, max_m, periodic, radius), never its lists."""
import numpy as np

from xmhw_amd.displacement import STAGE_FIELDS, di_range, pair_metrics, wrapped_di

_FAR = np.iinfo(np.int64).max
_BIAS = 1 << 15


def in_event(view, T):
    """(T, C) bool: cell c on step t lies in a table row (index_start <= t <= index_end)"""
    out = np.zeros((T, view["C"]), dtype=bool)
    cell = np.repeat(np.arange(view["C"]), np.diff(view["offsets"]))
    for c, s, e in zip(cell, view["start"], view["end"]):
        out[int(s):int(e) + 1, c] = True
    return out


def row_keys(table, j):
    """For grid row j and EVERY (dj, di) of the grid (rows x di_range): the combined key dist_m * 2**32 + (dj + 2**15) *
    2**16 + (di + 2**15) -- its order is that of (dist_m, dj, di) -- with _FAR beyond max_distance, and the metrics.
    Shape (ny, n_di)."""
    phi = np.deg2rad(table.lat)
    di = di_range(table.nx, table.periodic)
    dlam = np.deg2rad(di.astype(np.float64) * table.dlon)
    dist, north, east = pair_metrics(phi[j], phi[:, None], dlam[None, :], table.radius)
    dj = (np.arange(table.ny) - j)[:, None]
    key = dist * (1 << 32) + (dj + _BIAS) * (1 << 16) + (di[None, :] + _BIAS)
    return np.where(dist <= table.max_m, key, _FAR), dist, north, east


def brute_lists(table):
    """the candidate lists by exhaustive evaluation: per row (dj, di, dist_m, north_m, east_m) sorted by the key"""
    out = []
    di = di_range(table.nx, table.periodic)
    for j in range(table.ny):
        key, dist, north, east = row_keys(table, j)
        r, d = np.nonzero(key != _FAR)
        order = np.argsort(key[r, d], kind="stable")
        r, d = r[order], d[order]
        out.append((r - j, di[d], dist[r, d], north[r, d], east[r, d]))
    return out


def displacement_grid(field, seas, rows, view, cell_index, table, classes, K, basin=None, coldSpells=False, **_):
    """the stage of xmhw_amd.displacement.displacement_grid(): a dict of STAGE_FIELDS (K, C) and n_visited"""
    field = np.asarray(field)
    T, N = field.shape
    ny, nx = table.ny, table.nx
    assert N == ny * nx
    C = int(view["C"])
    x = field.astype(np.float64).reshape(T, ny, nx)
    if coldSpells:
        x = -x
    seas = np.asarray(seas, dtype=np.float64)
    ev = in_event(view, T)
    cell_of_point = np.full(N, -1, dtype=np.int64)
    cell_of_point[np.asarray(cell_index)] = np.arange(C)
    cgrid = cell_of_point.reshape(ny, nx)
    bgrid = None if basin is None else np.asarray(basin).reshape(ny, nx).astype(np.int64)
    di0 = int(di_range(nx, table.periodic)[0])
    cols = np.arange(nx)
    out = {"n_days": np.zeros((K, C), np.int32), "n_found": np.zeros((K, C), np.int32), "max_m": np.zeros((K, C), np.int32),
           "sum_m": np.zeros((K, C), np.int64), "sum_north_m": np.zeros((K, C), np.int64),
           "sum_east_m": np.zeros((K, C), np.int64)}
    n_visited = 0
    for j in range(ny):
        key, dist, north, east = row_keys(table, j)
        listed = np.sort(key[key != _FAR])                                   # the keys of row j's list, for n_visited
        ocean = np.nonzero(cgrid[j] >= 0)[0]
        if bgrid is not None:
            ocean = ocean[bgrid[j, ocean] >= 0]
        if not ocean.size:
            continue
        for t in range(T):
            k = int(classes[t])
            if k < 0:
                continue
            src = ocean[ev[t, cgrid[j, ocean]]]                              # the source columns of row j on day t
            if not src.size:
                continue
            c = cgrid[j, src]
            g = seas[rows[t], c]
            d_idx = wrapped_di(src[:, None], cols[None, :], nx, table.periodic) - di0           # (S, nx)
            keys = key[:, d_idx].transpose(1, 0, 2)                           # (S, ny, nx): every grid point's key
            with np.errstate(invalid="ignore"):
                q = x[t][None, :, :] <= g[:, None, None]                      # NaN compares false
            if bgrid is not None:
                q &= bgrid[None, :, :] == bgrid[j, src][:, None, None]
            keys = np.where(q, keys, _FAR).reshape(src.size, -1)
            best = keys.argmin(axis=1)
            kbest = keys[np.arange(src.size), best]
            found = kbest != _FAR
            jj, ii = np.unravel_index(best, (ny, nx))
            dd = d_idx[np.arange(src.size), ii]
            np.add.at(out["n_days"][k], c, 1)
            f = np.nonzero(found)[0]
            np.add.at(out["n_found"][k], c[f], 1)
            np.add.at(out["sum_m"][k], c[f], dist[jj[f], dd[f]])
            np.add.at(out["sum_north_m"][k], c[f], north[jj[f], dd[f]])
            np.add.at(out["sum_east_m"][k], c[f], east[jj[f], dd[f]])
            np.maximum.at(out["max_m"][k], c[f], dist[jj[f], dd[f]].astype(np.int32))
            n_visited += int((np.searchsorted(listed, kbest[f]) + 1).sum()) + int((~found).sum()) * listed.size
    assert set(out) == set(STAGE_FIELDS)
    out["n_visited"] = n_visited
    return out
