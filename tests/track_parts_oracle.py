"""mhw_track_parts() restated by brute force: the definition the device is compared with.

For every selected object and every day of its life the footprint -- the cells that hold a table row of the object
covering the day -- is rasterised into a dense (ny, nx) boolean map and flood-filled with an explicit stack in plain
Python; the 4 or 8 neighbours and the wrap along one axis are computed here, not taken from xmhw_amd's neighbour
table; part sizes and weights are summed with Python integers.  On purpose it knows nothing of union-find or voxel
numbers.

* parts_of_map(): the parts of one boolean map -> (cells, area) per part.
* parts_dense(): the public function restated from an EventDataset and an ObjectDataset.
* stage_oracle(): a function with the signature of xmhw_amd.track_parts.track_parts_device for one grid, the stand-in
  for the device in the host tests; it ignores the neighbour table and the voxel offsets it is handed.
"""
import numpy as np

import tracks_oracle as to

STEPS4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
STEPS8 = STEPS4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def parts_of_map(on, weight, neighbours, periodic_axis=None):
    """``on`` (ny, nx) bool, ``weight`` (ny, nx) of Python-int-convertible weights -> [(cells, area), ...], one per
    connected component under 4 or 8 neighbours, ``periodic_axis`` (0, 1 or None) wrapping"""
    ny, nx = on.shape
    steps = STEPS4 if neighbours == 4 else STEPS8
    seen = np.zeros((ny, nx), dtype=bool)
    out = []
    for i0, j0 in zip(*np.nonzero(on)):
        if seen[i0, j0]:
            continue
        seen[i0, j0] = True
        stack, cells, area = [(int(i0), int(j0))], 0, 0
        while stack:
            i, j = stack.pop()
            cells += 1
            area += int(weight[i, j])
            for di, dj in steps:
                ii, jj = i + di, j + dj
                if periodic_axis == 0:
                    ii %= ny
                if periodic_axis == 1:
                    jj %= nx
                if 0 <= ii < ny and 0 <= jj < nx and on[ii, jj] and not seen[ii, jj]:
                    seen[ii, jj] = True
                    stack.append((ii, jj))
        out.append((cells, area))
    return out


def _series(start, end, flat, member, t0, t1, sshape, wq_grid, neighbours, periodic_axis):
    """the three lists of one object whose rows are ``member`` (indices), living from t0 to t1"""
    ny, nx = sshape
    n_parts, cells_largest, area_largest = [], [], []
    for t in range(t0, t1 + 1):
        on = np.zeros((ny, nx), dtype=bool)
        for r in member:
            if start[r] <= t <= end[r]:
                on[flat[r] // nx, flat[r] % nx] = True
        parts = parts_of_map(on, wq_grid, neighbours, periodic_axis)
        n_parts.append(len(parts))
        cells_largest.append(max((p[0] for p in parts), default=0))
        area_largest.append(max((p[1] for p in parts), default=0))
    return n_parts, cells_largest, area_largest


def parts_dense(ds, obj, ids=None, weights=None, neighbours=None):
    """dict of flat lists in CSR order: offsets, n_parts, cells_largest, area_largest_q, and per object n_parts_max,
    pos_n_parts_max, days_split; ``neighbours`` None -> 4 for obj.connectivity 6, 8 for 26"""
    ny, nx = (int(v) for v in ds.sshape)
    ids = list(range(obj.n_objects)) if ids is None else [int(i) for i in ids]
    neighbours = neighbours or (4 if obj.connectivity == 6 else 8)
    axis = None if obj.periodic is None else list(ds.sdims).index(obj.periodic)
    w = to.grid_weights(ds, weights)
    wq = np.array([int(v) for v in np.rint(w / float(w.max()) * 2 ** int(obj.weight_bits))], dtype=object).reshape(ny, nx)
    flat = np.asarray(ds.cell_index)[np.repeat(np.arange(int(ds.n_cells)), np.diff(ds.offsets))]
    start = ds.table[:, to.COL_START].astype(np.int64)
    end = ds.table[:, to.COL_END].astype(np.int64)
    out = {k: [] for k in ("n_parts", "cells_largest", "area_largest_q", "n_parts_max", "pos_n_parts_max", "days_split")}
    offsets = [0]
    for o in ids:
        t0, t1 = int(obj.time_start[o]), int(obj.time_end[o])
        member = [int(r) for r in np.nonzero(np.asarray(obj.object) == o)[0]]
        a, b, c = _series(start, end, flat, member, t0, t1, (ny, nx), wq, neighbours, axis)
        out["n_parts"] += a
        out["cells_largest"] += b
        out["area_largest_q"] += c
        out["n_parts_max"].append(max(a))
        out["pos_n_parts_max"].append(t0 + a.index(max(a)))
        out["days_split"].append(sum(1 for v in a if v > 1))
        offsets.append(offsets[-1] + len(a))
    out.update(offsets=offsets, ids=ids, neighbours=neighbours)
    return out


def stage_oracle(cell_index, sshape, neighbours, periodic_axis=None):
    """a stand-in for track_parts_device() on the grid ``sshape`` whose compact cell c is the flat grid point
    cell_index[c]"""
    cell_index = np.asarray(cell_index, dtype=np.int64)
    ny, nx = (int(v) for v in sshape)

    def stage(start, end, slot, cell, row_offsets, nbr, wq, vox_off, time_start, offsets):
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        slot, offsets = np.asarray(slot, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
        flat = cell_index[np.asarray(cell, dtype=np.int64)]
        wq_grid = np.zeros(ny * nx, dtype=object)
        wq_grid[cell_index] = [int(v) for v in wq]
        wq_grid = wq_grid.reshape(ny, nx)
        m = offsets.shape[0] - 1
        out = ([], [], [])
        for i in range(m):
            t0 = int(time_start[i])
            t1 = t0 + int(offsets[i + 1] - offsets[i]) - 1
            member = [int(r) for r in np.nonzero(slot == i)[0]]
            for lst, add in zip(out, _series(start, end, flat, member, t0, t1, (ny, nx), wq_grid, neighbours, periodic_axis)):
                lst += add
        return dict(n_parts=np.array(out[0], dtype=np.int32).reshape(-1), cells_largest=np.array(out[1], dtype=np.int32).reshape(-1),
                    area_largest_q=np.array([int(v) for v in out[2]], dtype=np.int64).reshape(-1))

    return stage


def stage_for(ds, obj, neighbours=None):
    """stage_oracle() for the grid of ``ds`` with the wrap of ``obj`` and ``neighbours`` as mhw_track_parts() reads it"""
    neighbours = neighbours or (4 if obj.connectivity == 6 else 8)
    axis = None if obj.periodic is None else list(ds.sdims).index(obj.periodic)
    return stage_oracle(ds.cell_index, ds.sshape, neighbours, axis)


def same_as_dense(tp, want):
    """every integer of a TrackPartsDataset equal to parts_dense()'s"""
    import numpy.testing as npt
    npt.assert_array_equal(tp.offsets, np.asarray(want["offsets"], dtype=np.int64))
    assert tp.neighbours == want["neighbours"]
    assert tp.n_parts.dtype == np.int32 and tp.cells_largest.dtype == np.int32 and tp.area_largest_q.dtype == np.int64
    for k in ("n_parts", "cells_largest", "area_largest_q", "n_parts_max", "pos_n_parts_max", "days_split"):
        npt.assert_array_equal(getattr(tp, k), np.asarray(want[k], dtype=np.int64), err_msg=k)
