"""mhw_track_genealogy() restated by brute force: the definition the device is compared with.

The definition.  The parts of a selected object on one of its days are the connected components of its footprint --
the cells that hold a table row of the object covering the day -- under 4 or 8 neighbours, one axis wrapping or none.
The label of a part is the smallest flat grid index of its cells.  Part A of day t - 1 and part B of day t are linked
iff some cell lies in A on t - 1 and in B on t.  The edges are the distinct links; the in-degree of a part counts its
links to the day before, the out-degree those to the day after.  Per day: n_parts, n_links (the sum of the
in-degrees), n_born (in-degree 0), n_merged (in-degree >= 2), n_ended (out-degree 0), n_split (out-degree >= 2).

How.  Every selected object and day is rasterised into a dense (ny, nx) boolean map and flood-filled with an explicit
stack in plain Python into a label map (-1 off the footprint), with 4 / 8 steps and a wrap computed here; for two
consecutive days the links are the Python ``set`` of (label_before[c], label_after[c]) over the cells on in both
maps, and the degrees are counted from that set.  On purpose it knows nothing of union-find, voxel numbers or hash
tables.

* label_map(): one boolean map -> its label map.
* genealogy_dense(): the public function restated from an EventDataset and an ObjectDataset.
* stage_oracle() / stage_for(): a function with the signature of xmhw_amd.track_genealogy.track_genealogy_device for
  one grid, the stand-in for the device in the host tests; it ignores the neighbour table and the voxel offsets it is
  handed.
"""
import numpy as np

FIELDS = ("n_parts", "n_links", "n_born", "n_merged", "n_ended", "n_split")
STEPS4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
STEPS8 = STEPS4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))
COL_START, COL_END = 1, 2                                        # index_start, index_end of EventDataset.columns (checked below)


def label_map(on, neighbours, periodic_axis=None):
    """``on`` (ny, nx) bool -> (ny, nx) int64: the smallest flat index of the cell's component, -1 where off"""
    ny, nx = on.shape
    steps = STEPS4 if neighbours == 4 else STEPS8
    lab = np.full((ny, nx), -1, dtype=np.int64)
    for i0 in range(ny):                                          # row-major: the first cell met is the smallest
        for j0 in range(nx):
            if not on[i0, j0] or lab[i0, j0] >= 0:
                continue
            name = i0 * nx + j0
            lab[i0, j0] = name
            stack = [(i0, j0)]
            while stack:
                i, j = stack.pop()
                for di, dj in steps:
                    ii, jj = i + di, j + dj
                    if periodic_axis == 0:
                        ii %= ny
                    if periodic_axis == 1:
                        jj %= nx
                    if 0 <= ii < ny and 0 <= jj < nx and on[ii, jj] and lab[ii, jj] < 0:
                        lab[ii, jj] = name
                        stack.append((ii, jj))
    return lab


def _object(start, end, flat, member, t0, t1, sshape, neighbours, periodic_axis):
    """one object whose rows are ``member`` (indices), living from t0 to t1: (the six lists, one value a day; the
    edges as a sorted list of (t of the later day, label before, label after))"""
    ny, nx = sshape
    maps = []
    for t in range(t0, t1 + 1):
        on = np.zeros((ny, nx), dtype=bool)
        for r in member:
            if start[r] <= t <= end[r]:
                on[flat[r] // nx, flat[r] % nx] = True
        maps.append(label_map(on, neighbours, periodic_axis))
    links = [set()]                                               # links[d]: between day d - 1 and day d
    for before, after in zip(maps[:-1], maps[1:]):
        both = (before >= 0) & (after >= 0)
        links.append({(int(a), int(b)) for a, b in zip(before[both], after[both])})
    links.append(set())
    out = {k: [] for k in FIELDS}
    edges = []
    for d, lab in enumerate(maps):
        names = sorted({int(v) for v in lab[lab >= 0]})
        indeg, outdeg = {v: 0 for v in names}, {v: 0 for v in names}
        for a, b in links[d]:
            indeg[b] += 1
        for a, b in links[d + 1]:
            outdeg[a] += 1
        out["n_parts"].append(len(names))
        out["n_links"].append(len(links[d]))
        out["n_born"].append(sum(1 for v in names if indeg[v] == 0))
        out["n_merged"].append(sum(1 for v in names if indeg[v] >= 2))
        out["n_ended"].append(sum(1 for v in names if outdeg[v] == 0))
        out["n_split"].append(sum(1 for v in names if outdeg[v] >= 2))
        edges += [(t0 + d, a, b) for a, b in sorted(links[d])]
    return out, edges


def genealogy_dense(ds, obj, ids=None, neighbours=None):
    """dict of flat lists in CSR order: offsets, the six FIELDS, the sorted edges (edge_track, edge_pos, edge_from,
    edge_to with labels), edge_offsets, and per object n_splits, n_merges, n_births, n_ends, n_nodes, n_edges"""
    assert ds.columns.index("index_start") == COL_START and ds.columns.index("index_end") == COL_END
    ny, nx = (int(v) for v in ds.sshape)
    ids = list(range(obj.n_objects)) if ids is None else [int(i) for i in ids]
    neighbours = neighbours or (4 if obj.connectivity == 6 else 8)
    axis = None if obj.periodic is None else list(ds.sdims).index(obj.periodic)
    flat = np.asarray(ds.cell_index)[np.repeat(np.arange(int(ds.n_cells)), np.diff(ds.offsets))]
    start = ds.table[:, COL_START].astype(np.int64)
    end = ds.table[:, COL_END].astype(np.int64)
    out = {k: [] for k in FIELDS + ("edge_track", "edge_pos", "edge_from", "edge_to", "n_splits", "n_merges", "n_births",
                                    "n_ends", "n_nodes", "n_edges")}
    offsets, edge_offsets = [0], [0]
    for i, o in enumerate(ids):
        t0, t1 = int(obj.time_start[o]), int(obj.time_end[o])
        member = [int(r) for r in np.nonzero(np.asarray(obj.object) == o)[0]]
        series, edges = _object(start, end, flat, member, t0, t1, (ny, nx), neighbours, axis)
        for k in FIELDS:
            out[k] += series[k]
        for t, a, b in edges:
            out["edge_track"].append(i)
            out["edge_pos"].append(t)
            out["edge_from"].append(a)
            out["edge_to"].append(b)
        out["n_splits"].append(sum(series["n_split"]))
        out["n_merges"].append(sum(series["n_merged"]))
        out["n_births"].append(sum(series["n_born"][1:]))
        out["n_ends"].append(sum(series["n_ended"][:-1]))
        out["n_nodes"].append(sum(series["n_parts"]))
        out["n_edges"].append(len(edges))
        offsets.append(offsets[-1] + len(series["n_parts"]))
        edge_offsets.append(edge_offsets[-1] + len(edges))
    out.update(offsets=offsets, edge_offsets=edge_offsets, ids=ids, neighbours=neighbours)
    return out


def stage_oracle(cell_index, sshape, neighbours, periodic_axis=None):
    """a stand-in for track_genealogy_device() on the grid ``sshape`` whose compact cell c is the flat grid point
    cell_index[c]; like the device it names a part by its smallest COMPACT cell"""
    cell_index = np.asarray(cell_index, dtype=np.int64)
    ny, nx = (int(v) for v in sshape)
    compact = {int(f): c for c, f in enumerate(cell_index)}

    def stage(start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets):
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        slot, offsets = np.asarray(slot, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
        flat = cell_index[np.asarray(cell, dtype=np.int64)]
        out = {k: [] for k in FIELDS}
        rows = []
        for i in range(offsets.shape[0] - 1):
            t0 = int(time_start[i])
            t1 = t0 + int(offsets[i + 1] - offsets[i]) - 1
            member = [int(r) for r in np.nonzero(slot == i)[0]]
            series, edges = _object(start, end, flat, member, t0, t1, (ny, nx), neighbours, periodic_axis)
            for k in FIELDS:
                out[k] += series[k]
            rows += [(i, t, compact[a], compact[b]) for t, a, b in edges]
        got = {k: np.array(out[k], dtype=np.int32).reshape(-1) for k in FIELDS}
        rows = np.array(sorted(rows), dtype=np.int32).reshape(-1, 4)
        got.update(edge_track=rows[:, 0].copy(), edge_pos=rows[:, 1].copy(), edge_from=rows[:, 2].copy(), edge_to=rows[:, 3].copy())
        return got

    return stage


def stage_for(ds, obj, neighbours=None):
    """stage_oracle() for the grid of ``ds`` with the wrap of ``obj`` and ``neighbours`` as mhw_track_genealogy() reads it"""
    neighbours = neighbours or (4 if obj.connectivity == 6 else 8)
    axis = None if obj.periodic is None else list(ds.sdims).index(obj.periodic)
    return stage_oracle(ds.cell_index, ds.sshape, neighbours, axis)


PER_OBJECT = ("n_splits", "n_merges", "n_births", "n_ends", "n_nodes", "n_edges")
EDGES = ("edge_track", "edge_pos", "edge_from", "edge_to")


def same_as_dense(tg, want):
    """every integer and every edge of a TrackGenealogyDataset equal to genealogy_dense()'s"""
    import numpy.testing as npt
    npt.assert_array_equal(tg.offsets, np.asarray(want["offsets"], dtype=np.int64))
    npt.assert_array_equal(tg.edge_offsets, np.asarray(want["edge_offsets"], dtype=np.int64))
    assert tg.neighbours == want["neighbours"]
    assert all(getattr(tg, k).dtype == np.int32 for k in FIELDS + ("edge_track", "edge_pos"))
    assert tg.edge_from.dtype == np.int64 and tg.edge_to.dtype == np.int64 and tg.edge_offsets.dtype == np.int64
    for k in FIELDS + EDGES + PER_OBJECT:
        npt.assert_array_equal(getattr(tg, k), np.asarray(want[k], dtype=np.int64), err_msg=k)
