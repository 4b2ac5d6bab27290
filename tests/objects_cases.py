"""Inputs shared by the host and the GPU tests of mhw_objects(): EventDatasets built from interval lists, seeded
random grids with land, the golden event tables on a 9 x 12 grid, and synthetic CSR interval tables."""
import os

import numpy as np

from xmhw_amd.detect import EventDataset

GOLD = os.path.join(os.path.dirname(__file__), "golden")
COL = {k: EventDataset.columns.index(k) for k in EventDataset.columns}
SDIMS = ("lat", "lon")

# the issue's table: (connectivity, periodic) -> (objects, rows of the largest, single-row objects)
GOLDEN_COUNTS = {(6, None): (296, 236, 95), (26, None): (190, 587, 87), (6, "lon"): (273, 516, 95),
                 (26, "lon"): (161, 874, 87)}


def table_from(start, end, imax=None):
    n = len(start)
    tab = np.zeros((n, len(EventDataset.columns)))
    tab[:, COL["index_start"]] = tab[:, COL["time_start"]] = tab[:, COL["time_peak"]] = start
    tab[:, COL["index_end"]] = tab[:, COL["time_end"]] = end
    tab[:, COL["duration"]] = np.asarray(end) - np.asarray(start) + 1
    tab[:, COL["intensity_max"]] = np.arange(n) % 7 + 0.5 if imax is None else imax
    return tab


def dataset(sshape, keep, per_cell, T=None):
    """per_cell: for every ocean cell in stacked order a list of (start, end) or (start, end, intensity_max)"""
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    assert len(per_cell) == int(keep.sum())
    rows = [r for cell in per_cell for r in cell]
    start = np.array([r[0] for r in rows], dtype=np.int64)
    end = np.array([r[1] for r in rows], dtype=np.int64)
    imax = np.array([r[2] if len(r) > 2 else (k % 7 + 0.5) for k, r in enumerate(rows)], dtype=np.float64)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in per_cell])]).astype(np.int64)
    T = int(T if T is not None else (end.max() + 1 if len(rows) else 1))
    time = np.datetime64("2001-01-01") + np.arange(T)
    coords = {"lat": np.linspace(-60, 60, sshape[0]) if sshape[0] > 1 else np.zeros(1), "lon": np.arange(sshape[1]) * 1.0,
              "time": time}
    return EventDataset(table_from(start, end, imax), offsets, time, np.nonzero(keep)[0], keep, SDIMS, tuple(sshape), coords,
                        {}, {}, {}, False)


def random_intervals(rng, T, mean_rows):
    """disjoint runs in [0, T), at least one free day between them, in time order"""
    out, t = [], int(rng.integers(0, 6))
    while True:
        d = int(rng.integers(1, 8))
        if t + d > T or rng.random() < 1.0 / (mean_rows + 1):
            return out
        out.append((t, t + d - 1))
        t += d + int(rng.integers(1, 7))


def random_grid(seed, T=40):
    rng = np.random.default_rng(seed)
    ny, nx = int(rng.integers(2, 9)), int(rng.integers(3, 10))
    keep = rng.random(ny * nx) >= 0.2
    if not keep.any():
        keep[0] = True
    per_cell = [random_intervals(rng, T, 4) for _ in range(int(keep.sum()))]
    ds = dataset((ny, nx), keep, per_cell, T)
    ds.table[:, COL["intensity_max"]] = np.round(rng.normal(size=ds.n_events), 1)       # ties
    ds.table[rng.random(ds.n_events) < 0.1, COL["intensity_max"]] = np.nan
    return ds


def golden_dataset():
    g = np.load(os.path.join(GOLD, "mhw_features_cases.npz"))
    table, offsets = np.array(g["table"], dtype=np.float64), g["table_offsets"].astype(np.int64)
    assert offsets.shape[0] - 1 == 108 and table.shape[0] == 1795
    T = int(table[:, COL["index_end"]].max()) + 1
    time = np.datetime64("1982-01-01") + np.arange(T)
    keep = np.ones(108, dtype=bool)
    coords = {"lat": np.linspace(-40, 40, 9), "lon": np.arange(12) * 30.0, "time": time}
    return EventDataset(table, offsets, time, np.arange(108), keep, SDIMS, (9, 12), coords, {}, {}, {}, False)


def stage_inputs(ds, connectivity, periodic):
    """the compact arrays mhw_objects() hands to its device stage, and what the voxel route needs"""
    from xmhw_amd.objects import neighbour_table
    start = ds.table[:, COL["index_start"]].astype(np.int32)
    end = ds.table[:, COL["index_end"]].astype(np.int32)
    imax = np.ascontiguousarray(ds.table[:, COL["intensity_max"]])
    axis = None if periodic is None else ds.sdims.index(periodic)
    nbr = neighbour_table(ds.cell_index, ds.sshape, connectivity, axis)
    flat = np.asarray(ds.cell_index)[np.repeat(np.arange(ds.n_cells), np.diff(ds.offsets))]
    return start, end, imax, np.asarray(ds.offsets, dtype=np.int64), nbr, (0 if connectivity == 6 else 1), flat, axis


def csr_case(sizes, seed, T=4000, grid=None, land=0.0, connectivity=6, periodic_axis=None):
    """a synthetic CSR interval table: cell c has sizes[c] random disjoint runs; cells laid row-major on `grid`
    (default: one line of cells), a share `land` of the grid points left out.  Returns the stage arguments."""
    from xmhw_amd.objects import neighbour_table
    rng = np.random.default_rng(seed)
    C = len(sizes)
    if grid is None:
        grid = (1, C)
    N = grid[0] * grid[1]
    if land:
        keep = np.zeros(N, dtype=bool)
        keep[rng.choice(N, C, replace=False)] = True
    else:
        assert N == C
        keep = np.ones(N, dtype=bool)
    cell_index = np.nonzero(keep)[0]
    start, end = [], []
    for s in sizes:
        if s == 0:
            continue
        span = max(T, 6 * s)
        cuts = np.sort(rng.choice(span // 2, 2 * s, replace=False)) * 2     # even positions: runs end >= 1 day apart
        start.append(cuts[0::2])
        end.append(cuts[1::2] - 2)
    start = np.concatenate(start).astype(np.int32) if start else np.zeros(0, np.int32)
    end = np.concatenate(end).astype(np.int32) if end else np.zeros(0, np.int32)
    n = start.shape[0]
    imax = np.round(rng.normal(size=n), 1)
    imax[rng.random(n) < 0.05] = np.nan
    imax[rng.random(n) < 0.05] = -0.0
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    nbr = neighbour_table(cell_index, grid, connectivity, periodic_axis)
    wq = rng.integers(0, 1 << 20, C).astype(np.int64)
    return start, end, imax, offsets, nbr, (0 if connectivity == 6 else 1), wq
