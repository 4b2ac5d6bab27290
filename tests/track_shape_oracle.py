"""mhw_track_shape() restated by brute force: the definition the device is compared with.

For every selected object and every day of its life the footprint -- the cells that hold a table row of the object
covering the day -- is rasterised into a dense (ny, nx) boolean map beside the ocean mask; for each of the four
directions the map of what lies across the face is made by shifting both (with the wrap, the fold of a wrapping dim of
length 1 and the edge of the grid handled here, not taken from xmhw_amd's face table), every face of every footprint
cell is put into its class, and counts and lengths are summed with Python integers.  On purpose it knows nothing of row
searches, cursors or atomics.

* faces_of_map(): the classes of the faces of one boolean map.
* sphere_lengths() / quantised(): the "sphere" lengths and the quantisation, with ``math`` loops over the coordinates.
* shape_dense(): the public function restated from an EventDataset and an ObjectDataset.
* stage_oracle(): a function with the signature of xmhw_amd.track_shape.track_shape_device for one grid, the stand-in
  for the device in the host tests; it ignores the face table and the row offsets it is handed.
"""
import math

import numpy as np

import tracks_oracle as to

STEPS = ((-1, 0), (1, 0), (0, -1), (0, 1))                       # dim 0 minus, dim 0 plus, dim 1 minus, dim 1 plus
FIELDS = ("edges_open", "edges_coast", "edges_border", "perimeter_open_q", "perimeter_coast_q", "perimeter_border_q",
          "cells_edge")
R_KM = 6371.0088


def _across(a, axis, step, wraps):
    """(the value of ``a`` one ``step`` along ``axis`` from every point, whether there is a point there)"""
    if wraps:
        return np.roll(a, -step, axis=axis), np.ones(a.shape, dtype=bool)
    out, there = np.zeros_like(a), np.zeros(a.shape, dtype=bool)
    src = [slice(None), slice(None)]
    dst = [slice(None), slice(None)]
    src[axis] = slice(1, None) if step == 1 else slice(None, -1)
    dst[axis] = slice(None, -1) if step == 1 else slice(1, None)
    out[tuple(dst)] = a[tuple(src)]
    there[tuple(dst)] = True
    return out, there


def faces_of_map(on, ocean, periodic_axis=None):
    """``on``, ``ocean`` (ny, nx) bool -> [(open, coast, border), ...] for the four directions, each a (ny, nx) bool map of
    the footprint cells whose face in that direction is of that class; a folded direction gives three empty maps"""
    out = []
    for di, dj in STEPS:
        axis, step = (0, di) if di else (1, dj)
        wraps = periodic_axis == axis
        if wraps and on.shape[axis] == 1:                        # folded: the cell across is the cell itself
            out.append((np.zeros_like(on), np.zeros_like(on), np.zeros_like(on)))
            continue
        on_there, there = _across(on, axis, step, wraps)
        ocean_there, _ = _across(ocean, axis, step, wraps)
        out.append((on & there & ocean_there & ~on_there, on & there & ~ocean_there, on & ~there))
    return out


def _series(start, end, flat, member, t0, t1, ocean, lq_grid, periodic_axis):
    """the seven lists of one object whose rows are ``member`` (indices), living from t0 to t1; lq_grid (ny, nx, 4) object"""
    ny, nx = ocean.shape
    out = {k: [] for k in FIELDS}
    for t in range(t0, t1 + 1):
        on = np.zeros((ny, nx), dtype=bool)
        for r in member:
            if start[r] <= t <= end[r]:
                on[flat[r] // nx, flat[r] % nx] = True
        assert not (on & ~ocean).any()
        count, length, any_face = [0, 0, 0], [0, 0, 0], np.zeros((ny, nx), dtype=bool)
        for k, classes in enumerate(faces_of_map(on, ocean, periodic_axis)):
            for c, mask in enumerate(classes):
                count[c] += int(mask.sum())
                length[c] += sum(int(v) for v in lq_grid[:, :, k][mask])
                any_face |= mask
        for c, name in enumerate(("open", "coast", "border")):
            out[f"edges_{name}"].append(count[c])
            out[f"perimeter_{name}_q"].append(length[c])
        out["cells_edge"].append(int(any_face.sum()))
    return out


def _edges(x, clip=None):
    e = [x[0] - 0.5 * (x[1] - x[0])] + [0.5 * (x[i] + x[i + 1]) for i in range(len(x) - 1)] + [x[-1] + 0.5 * (x[-1] - x[-2])]
    return e if clip is None else [min(max(v, -clip), clip) for v in e]


def sphere_lengths(ds):
    """(ny, nx, 4) float64 km, from the 1-D coordinates of ``ds`` in degrees"""
    names = to._names(ds)
    assert names is not None
    a_lat = list(ds.sdims).index(names[0])
    lat = [float(v) for v in np.asarray(ds.coords[names[0]], dtype=np.float64)]
    lon = [float(v) for v in np.asarray(ds.coords[names[1]], dtype=np.float64)]
    e_lat, e_lon = _edges(lat, 90.0), _edges(lon)
    cos_face = [0.0 if abs(v) >= 90.0 else max(float(np.cos(np.float64(math.radians(v)))), 0.0) for v in e_lat]
    dphi = [abs(math.radians(e_lat[i + 1]) - math.radians(e_lat[i])) for i in range(len(lat))]
    dlam = [abs(math.radians(e_lon[j + 1]) - math.radians(e_lon[j])) for j in range(len(lon))]
    out = np.zeros(tuple(ds.sshape) + (4,))
    for i in range(ds.sshape[0]):
        for j in range(ds.sshape[1]):
            p, q = (i, j) if a_lat == 0 else (j, i)              # p along the latitude, q along the longitude
            along_lat = [(R_KM * cos_face[p]) * dlam[q], (R_KM * cos_face[p + 1]) * dlam[q]]      # across the lat dim
            along_lon = [R_KM * dphi[p]] * 2
            out[i, j] = along_lat + along_lon if a_lat == 0 else along_lon + along_lat
    return out


def bits_for(n_ocean):
    return min(31, 60 - int(n_ocean).bit_length())


def quantised(ln, bits):
    """(ny, nx, 4) object array of Python ints, and the unit"""
    top = float(ln.max())
    q = np.empty(ln.shape, dtype=object)
    for idx in np.ndindex(*ln.shape):
        q[idx] = int(round(float(ln[idx]) / top * float(1 << bits)))     # round(): half to even, as rint
    return q, top / float(1 << bits)


def grid_lengths(ds, lengths):
    if lengths is None:
        return np.ones(tuple(ds.sshape) + (4,))
    if isinstance(lengths, str):
        return sphere_lengths(ds)
    return np.asarray(lengths, dtype=np.float64)


def shape_dense(ds, obj, ids=None, lengths=None):
    """dict of flat lists in CSR order: offsets, the seven stage fields, and per object perimeter_max_q,
    pos_perimeter_max, days_coastal; length_bits and length_unit"""
    ny, nx = (int(v) for v in ds.sshape)
    ids = list(range(obj.n_objects)) if ids is None else [int(i) for i in ids]
    axis = None if obj.periodic is None else list(ds.sdims).index(obj.periodic)
    bits = bits_for(ds.n_cells)
    lq, unit = quantised(grid_lengths(ds, lengths), bits)
    ocean = np.zeros(ny * nx, dtype=bool)
    ocean[np.asarray(ds.cell_index)] = True
    ocean = ocean.reshape(ny, nx)
    flat = np.asarray(ds.cell_index)[np.repeat(np.arange(int(ds.n_cells)), np.diff(ds.offsets))]
    start = ds.table[:, to.COL_START].astype(np.int64)
    end = ds.table[:, to.COL_END].astype(np.int64)
    out = {k: [] for k in FIELDS + ("perimeter_max_q", "pos_perimeter_max", "days_coastal")}
    offsets = [0]
    for o in ids:
        t0, t1 = int(obj.time_start[o]), int(obj.time_end[o])
        member = [int(r) for r in np.nonzero(np.asarray(obj.object) == o)[0]]
        s = _series(start, end, flat, member, t0, t1, ocean, lq, axis)
        for k in FIELDS:
            out[k] += s[k]
        total = [a + b + c for a, b, c in zip(s["perimeter_open_q"], s["perimeter_coast_q"], s["perimeter_border_q"])]
        out["perimeter_max_q"].append(max(total))
        out["pos_perimeter_max"].append(t0 + total.index(max(total)))
        out["days_coastal"].append(sum(1 for v in s["edges_coast"] if v > 0))
        offsets.append(offsets[-1] + len(total))
    out.update(offsets=offsets, ids=ids, length_bits=bits, length_unit=unit)
    return out


def stage_oracle(cell_index, sshape, periodic_axis=None):
    """a stand-in for track_shape_device() on the grid ``sshape`` whose compact cell c is the flat grid point
    cell_index[c]"""
    cell_index = np.asarray(cell_index, dtype=np.int64)
    ny, nx = (int(v) for v in sshape)

    def stage(start, end, slot, cell, row_offsets, faces, lq, time_start, offsets):
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        slot, offsets = np.asarray(slot, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
        flat = cell_index[np.asarray(cell, dtype=np.int64)]
        ocean = np.zeros(ny * nx, dtype=bool)
        ocean[cell_index] = True
        lq_grid = np.zeros((ny * nx, 4), dtype=object)
        for c, p in enumerate(cell_index):
            lq_grid[p] = [int(v) for v in np.asarray(lq)[c]]
        m = offsets.shape[0] - 1
        out = {k: [] for k in FIELDS}
        for i in range(m):
            t0 = int(time_start[i])
            t1 = t0 + int(offsets[i + 1] - offsets[i]) - 1
            member = [int(r) for r in np.nonzero(slot == i)[0]]
            s = _series(start, end, flat, member, t0, t1, ocean.reshape(ny, nx), lq_grid.reshape(ny, nx, 4), periodic_axis)
            for k in FIELDS:
                out[k] += s[k]
        return {k: np.array([int(v) for v in out[k]], dtype=np.int64 if k.endswith("_q") else np.int32).reshape(-1)
                for k in FIELDS}

    return stage


def stage_for(ds, obj):
    """stage_oracle() for the grid of ``ds`` with the wrap of ``obj``"""
    axis = None if obj.periodic is None else list(ds.sdims).index(obj.periodic)
    return stage_oracle(ds.cell_index, ds.sshape, axis)


def same_as_dense(ts, want):
    """every integer of a TrackShapeDataset equal to shape_dense()'s"""
    import numpy.testing as npt
    npt.assert_array_equal(ts.offsets, np.asarray(want["offsets"], dtype=np.int64))
    assert ts.length_bits == want["length_bits"] and ts.length_unit == want["length_unit"]
    for k in FIELDS:
        assert getattr(ts, k).dtype == (np.int64 if k.endswith("_q") else np.int32), k
        npt.assert_array_equal(getattr(ts, k), np.asarray(want[k], dtype=np.int64), err_msg=k)
    npt.assert_array_equal(ts.perimeter_max, np.asarray(want["perimeter_max_q"], dtype=np.int64) * want["length_unit"])
    npt.assert_array_equal(ts.pos_perimeter_max, np.asarray(want["pos_perimeter_max"], dtype=np.int64))
    npt.assert_array_equal(ts.days_coastal, np.asarray(want["days_coastal"], dtype=np.int64))
