"""Inputs shared by the host and the GPU tests of mhw_displacement().  TEST INFRASTRUCTURE ONLY.

stage_case() builds what the device stage takes: an uncompacted (T, ny * nx) field with land, a compact climatology, an
event table over the ocean cells (cooccurrence_cases.table: the sources do not depend on the field, gap days and
one-step rows included) and the DisplacementTable of the grid."""
import numpy as np

import cooccurrence_cases as coc
from xmhw_amd.displacement import displacement_offsets

D = 5                               # climatology rows; step t uses row (3 t + 1) % D


def land_mask(ny, nx, rng, land, land_row):
    """keep (ny, nx): ``land`` of the points are land, plus (land_row, ny >= 3) the whole row 1; point (0, 0) is ocean"""
    keep = rng.random((ny, nx)) >= land
    if land_row and ny >= 3:
        keep[1, :] = False
    keep[0, 0] = True
    return keep


def two_basins(ny, nx, keep):
    """(basin (ny, nx) int32, keep): a land bridge along the middle column splits basin 3 (west) from basin 7 (east); a
    few ocean points carry -1 (excluded) or -5"""
    keep = keep.copy()
    mid = nx // 2
    keep[:, mid] = False
    basin = np.where(np.arange(nx)[None, :] < mid, 3, 7).astype(np.int32) * np.ones((ny, 1), dtype=np.int32)
    basin[0, ::5] = -1
    basin[ny - 1, 1::7] = -5
    keep[0, 0] = True
    return basin, keep


def stage_case(ny, nx, T, seed=0, dtype=np.float32, land=0.3, land_row=True, holes=0.02, periodic=False,
               max_distance=600.0, cold=False, basin=False, classes=None, field="blobs", dlon=1.0):
    """dict(field (T, N), seas (D, C), rows (T,), view, cell_index (C,), table, classes (T,), K, basin, cold, keep)"""
    rng = np.random.default_rng(seed)
    N = ny * nx
    keep = land_mask(ny, nx, rng, land, land_row)
    bas = None
    if basin:
        bas, keep = two_basins(ny, nx, keep)
    lat = np.linspace(-32.0, 28.0, ny) + (0.3 * np.sin(np.arange(ny)) if ny > 2 else 0.0)      # irregular
    if ny == 1:
        lat = np.array([12.5])
    cell_index = np.nonzero(keep.reshape(-1))[0].astype(np.int64)
    C = cell_index.shape[0]
    jj, ii = np.divmod(np.arange(N), nx)
    clim = 18.0 - 0.25 * jj[None, :] + 0.4 * np.sin(np.arange(D))[:, None] + 0.2 * rng.standard_normal((D, N))
    rows = ((3 * np.arange(T) + 1) % D).astype(np.int32)
    if field == "blobs":                              # a warm blob that drifts over a noisy background
        j0 = (ny - 1) * (0.5 + 0.4 * np.sin(np.arange(T) / 7.0))
        i0 = (nx - 1) * (0.5 + 0.45 * np.cos(np.arange(T) / 11.0))
        r2 = (jj[None, :] - j0[:, None]) ** 2 + ((ii[None, :] - i0[:, None]) / 2.0) ** 2
        anom = 2.5 * np.exp(-r2 / (2.0 + 0.02 * N)) - 0.4 + 0.5 * rng.standard_normal((T, N))
    elif field == "warm":                             # uniformly warm: nothing qualifies anywhere
        anom = np.full((T, N), 3.0)
    elif field == "cool":                             # every source finds itself
        anom = np.full((T, N), -1.0)
    else:
        raise ValueError(field)
    sign = -1.0 if cold else 1.0
    x = (sign * (clim[rows] + anom)).astype(dtype)     # under coldSpells the stage negates the series back
    if holes:
        x[rng.random((T, N)) < holes] = np.nan
    x[:, ~keep.reshape(-1)] = np.nan
    seas = np.ascontiguousarray(clim[:, cell_index])
    if C > 3:
        seas[rows[0], 2] = np.nan                      # a NaN target: that source finds nothing
    view = coc.table(T, C, seed + 17)
    view["cell_index"] = cell_index
    if classes is None:
        classes, K = np.zeros(T, dtype=np.int32), 1
    else:
        classes, K = classes(T)
    table = displacement_offsets(lat, nx, dlon, max_distance, periodic)
    return dict(field=x, seas=seas, rows=rows, view=view, cell_index=cell_index, table=table, classes=classes, K=K,
                basin=None if bas is None else bas.reshape(-1), cold=cold, keep=keep)


def run_stage(stage, case, **extra):
    return stage(case["field"], case["seas"], case["rows"], case["view"], case["cell_index"], case["table"],
                 case["classes"], case["K"], basin=case["basin"], coldSpells=case["cold"], **extra)


def assert_same(got, want):
    from xmhw_amd.displacement import STAGE_FIELDS
    for name in STAGE_FIELDS:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
        assert got[name].dtype == want[name].dtype, name
    assert int(got["n_visited"]) == int(want["n_visited"])


def check_case(want, found=True, unreached=True, far=True):
    """On the oracle's side: the case has sources, and (as asked) found ones at a distance and unreached ones.  A case
    without them proves nothing."""
    assert want["n_days"].sum() > 0, "no source"
    if found:
        assert want["n_found"].sum() > 0, "nothing found"
    if far:
        assert want["max_m"].max() > 0, "every source found itself"
    if unreached:
        assert (want["n_days"] - want["n_found"]).sum() > 0, "every source was reached"
