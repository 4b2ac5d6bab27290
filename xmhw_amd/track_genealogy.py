"""mhw_track_genealogy(): which connected part of an object on one day continues into which part on the next day, and
the split and merge counts taken from it, aligned entry for entry with the ragged (CSR) arrays of mhw_tracks() and
mhw_track_parts(): entry offsets[i] + (t - time_start[i]) belongs to object ids[i] on time position t.
mhw_track_parts() says that an object is three patches on some day; this says whether they came from one patch that
broke up or are about to fuse.  The tracking tools of the field (Ocetrac, marEx) label a dense (time, lat, lon) volume
day by day and intersect the label maps; here the volume is never built: the voxels of the selected rows are numbered,
the lock-free union-find of mhw_track_parts() runs on them, and the (part, part) pairs of consecutive days are
deduplicated in a hash set on the device (csrc/kernels_genealogy.hip).

The definition.  Take a selected object o.
  * Parts.  The parts of o on day t are those of mhw_track_parts(): the connected components of its footprint (the
    ocean cells that hold a table row of o covering t) under ``neighbours`` (None: 4 for objects of connectivity 6, 8
    for 26; or 4 | 8), the grid wrapping along obj.periodic.  Parts never join cells of different objects.
  * Label.  The label of a part is the smallest flat grid index (cell_index[c]) of its cells.
  * Link.  Part A of day t - 1 and part B of day t of the same object are linked iff some cell lies in A on t - 1 and
    in B on t: overlap, the rule of Ocetrac and marEx.  A link through a diagonal or neighbouring cell is not counted,
    also for objects of connectivity 26.
  * Nodes and edges.  The nodes of the genealogy are the parts, its edges the distinct links.  A node of day t has an
    in-degree, its links to day t - 1, and an out-degree, its links to day t + 1.
Per entry, exact int32 counts over the parts of that day:
    n_parts     the number of parts (that of mhw_track_parts()),
    n_links     the sum of the in-degrees: the distinct links from the day before,
    n_born      parts with in-degree 0 (on an object's first day: all of them),
    n_merged    parts with in-degree >= 2,
    n_ended     parts with out-degree 0 (on the last day: all of them),
    n_split     parts with out-degree >= 2.
The edge list, E edges sorted by (edge_track, edge_pos, edge_from, edge_to): edge_track (int32) the position i in the
selection, edge_pos (int32) the position t of the LATER day, edge_from / edge_to (int64) the labels of A and B;
edge_offsets (m + 1,) holds the edges of each selected object.

Derived on the host, per selected object: n_splits = sum n_split, n_merges = sum n_merged, n_births = sum n_born over
all days but the first, n_ends = sum n_ended over all days but the last, n_nodes = sum n_parts, n_edges.

Identities: n_parts equals mhw_track_parts().n_parts; on the first day n_links == 0 and n_born == n_parts, on the last
n_ended == n_parts; the edges of (edge_track, edge_pos) number n_links of that entry; n_links >= n_parts - n_born; for
objects of connectivity 6, n_edges >= n_nodes - 1 (every union of mhw_objects() is then between rows of one cell or of
two cells adjacent under either ``neighbours``, so the genealogy is connected; under connectivity 26 a diagonal step in
time joins two rows that no overlap links).

Voxels are those of track_parts.voxel_offsets().  The device keeps 12 bytes per voxel (parent, in-degree, out-degree)
and 8 bytes per slot of the hash set, whose capacity is the smallest power of two >= 2 * max(edge_capacity, 1);
edge_capacity, computed exactly here, is the number of keys the device forms: the (row, day) pairs of the selected
rows with a next day in the row, plus the pairs of consecutive rows of one cell and object that touch in time.  The set
is therefore never more than half full.  V >= 2**31 is refused before anything is allocated.

Not here: links through neighbouring cells (their number has no tight bound from the table alone, so the set could not
be sized before the run); lineage ids (a walk of the returned edge list).

Host side here (validation, selection, neighbour table, voxel numbering, edge capacity, labels, sorting, the derived
fields); device side in csrc/kernels_genealogy.hip behind track_genealogy_device().
"""
import numpy as np

from .exception import XmhwException
from .objects import neighbour_table
from .track_common import ChainDataset, Selection, device_stage, stage_inputs
from .track_parts import voxel_offsets

COUNT_FIELDS = ("n_parts", "n_links", "n_born", "n_merged", "n_ended", "n_split")       # XMHW_GENEALOGY_* order
EDGE_FIELDS = ("edge_track", "edge_pos", "edge_from", "edge_to")
STAGE_FIELDS = COUNT_FIELDS + EDGE_FIELDS
_INPUTS = dict(start=np.int32, end=np.int32, slot=np.int32, cell=np.int32, row_offsets=np.int64, nbr=np.int32, vox_off=np.int64,
               time_start=np.int32, offsets=np.int64)
VOXEL_BYTES = 12                # XMHW_GENEALOGY_VOXEL_BYTES (include/xmhw_amd.h)
SLOT_BYTES = 8                  # XMHW_GENEALOGY_SLOT_BYTES


def edge_capacity(start, end, slot, cell):
    """The number of (part, part) keys the device forms: for every selected row its days but the last, plus the pairs of
    consecutive rows of one cell and slot with start == end + 1 (detect() emits none)."""
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    slot, cell = np.asarray(slot), np.asarray(cell)
    sel = slot >= 0
    within = int(np.maximum(end[sel] - start[sel], 0).sum())
    touching = sel[:-1] & (slot[1:] == slot[:-1]) & (cell[1:] == cell[:-1]) & (start[1:] == end[:-1] + 1)
    return within + int(touching.sum())


def table_slots(capacity):
    """the slots of the device's hash set for ``capacity`` keys: the smallest power of two >= 2 * max(capacity, 1)"""
    return 1 << (2 * max(int(capacity), 1) - 1).bit_length()


def sort_edges(track, pos, a, b):
    """the four edge arrays in the order (track, pos, from, to)"""
    order = np.lexsort((b, a, pos, track))
    return track[order], pos[order], a[order], b[order]


def edges_of_keys(keys, start, slot, cell, vox_off):
    """The device's edges, (root voxel of the earlier part << 32) | root voxel of the later part as uint64 in any order,
    as sorted (edge_track, edge_pos, edge_from, edge_to) int32 in compact cells.  A root is the smallest voxel of its
    part, a voxel of its smallest cell: its row follows from a search of vox_off, its day and cell from the row."""
    keys = np.asarray(keys, dtype=np.uint64)
    to_v = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    from_v = (keys >> np.uint64(32)).astype(np.int64)
    to_row = np.searchsorted(vox_off, to_v, side="right") - 1     # rows without voxels repeat an offset: the last one holds v
    from_row = np.searchsorted(vox_off, from_v, side="right") - 1
    pos = (np.asarray(start, dtype=np.int64)[to_row] + (to_v - np.asarray(vox_off)[to_row])).astype(np.int32)
    return sort_edges(np.asarray(slot, dtype=np.int32)[to_row], pos, np.asarray(cell, dtype=np.int32)[from_row],
                      np.asarray(cell, dtype=np.int32)[to_row])


def track_genealogy_device(start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets):
    """The device stage.  The arguments are those of track_parts_device() without the weights.  Returns a dict of
    STAGE_FIELDS: the six COUNT_FIELDS (L,) int32, L = offsets[-1], and the E edges sorted by (edge_track, edge_pos,
    edge_from, edge_to), all int32, edge_from / edge_to being the smallest COMPACT cell of the two parts
    (mhw_track_genealogy() turns them into labels with cell_index)."""
    start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets = a = stage_inputs(
        _INPUTS, start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets)
    n, m = start.shape[0], time_start.shape[0]
    L = int(offsets[-1])
    if L == 0 or n == 0 or m == 0:
        return {k: np.zeros(L if k in COUNT_FIELDS else 0, dtype=np.int32) for k in STAGE_FIELDS}
    C = row_offsets.shape[0] - 1
    if nbr.ndim != 2 or nbr.shape[0] != C or cell.shape != (n,) or vox_off.shape != (n + 1,):
        raise XmhwException("the neighbour table, the row offsets and the voxel offsets do not fit the rows and cells")
    V = int(vox_off[-1])
    cap = edge_capacity(start, end, slot, cell)
    F = len(COUNT_FIELDS)
    with device_stage(a, (n, m, L, V, C, cap), f"mhw_track_genealogy handles fewer than 2**31 rows, objects, series entries and "
                      f"voxels, got {n}, {m}, {L}, {V}") as (h, s, d, launch):
        with launch:
            d_counts, d_edges = s.alloc(4 * F * L), s.alloc(8 * max(cap, 1))
            d_ne, d_bad, d_over = s.alloc(8), s.alloc(4), s.alloc(4)
            h.object_genealogy(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, n, d[4].ptr, C, d[5].ptr, nbr.shape[1], d[6].ptr, V,
                               d[7].ptr, d[8].ptr, m, L, d_counts.ptr, d_edges.ptr, cap, d_ne.ptr, d_bad.ptr, d_over.ptr)
            h.stream_sync(0)
        counts = d_counts.to_array((F, L), np.int32)
        E = int(d_ne.to_array((1,), np.int64)[0])
        bad, over = int(d_bad.to_array((1,), np.int32)[0]), int(d_over.to_array((1,), np.int32)[0])
        keys = d_edges.to_array((max(cap, 1),), np.uint64)[:max(min(E, cap), 0)]
    if bad:
        raise XmhwException(f"{bad} table rows do not lie within their object's days, cells or voxels: obj does not belong "
                            "to mhw")
    if over or E > cap:
        raise XmhwException(f"the hash set of the genealogy stage overflowed ({E} edges, room for {cap}): the rows are not "
                            "in time order within their cells")
    out = {k: np.ascontiguousarray(counts[i]) for i, k in enumerate(COUNT_FIELDS)}
    track, pos, a, b = edges_of_keys(keys, start, slot, cell, vox_off)
    out.update(edge_track=track, edge_pos=pos, edge_from=a, edge_to=b)
    return out


class TrackGenealogyDataset(ChainDataset):
    """What mhw_track_genealogy() returns, as plain arrays, aligned with the TrackDataset / TrackPartsDataset of the same
    ``ids``: m objects, L = offsets[-1] entries; entry offsets[i] + (t - time_start[i]) belongs to object ids[i] on time
    position t.

    ids, offsets, time_start, time_end, duration, pos    as in the TrackDataset;
    n_parts, n_links, n_born, n_merged, n_ended, n_split (L,) int32     the counts of the module docstring;
    edge_track, edge_pos (E,) int32; edge_from, edge_to (E,) int64      the edges, sorted by these four in this order:
                                    the position of the object in the selection, the position of the later day, the
                                    labels (smallest flat grid index) of the earlier and of the later part;
    edge_offsets (m + 1,) int64     the edges of selected object i are edge_offsets[i] .. edge_offsets[i + 1] - 1;
    n_splits, n_merges, n_births, n_ends, n_nodes, n_edges (m,) int64  per object (module docstring);
    neighbours 4 | 8, periodic, n_voxels (V)."""

    _SERIES = ("pos",) + COUNT_FIELDS
    _PER_OBJECT = ("ids", "time_start", "time_end", "duration", "n_splits", "n_merges", "n_births", "n_ends", "n_nodes",
                   "n_edges")
    _ATTRS = ("neighbours", "periodic")

    def __init__(self, fields, time, sdims, sshape, neighbours, periodic, n_voxels, attrs=None):
        super().__init__(fields, time, sdims, sshape, attrs)
        self.neighbours, self.periodic, self.n_voxels = int(neighbours), periodic, int(n_voxels)

    def edges(self, i):
        """The edges of the i-th selected object: a dict of its slices of the four edge arrays plus ``time``, the stamps
        of the later days."""
        sl = self._span(i, "edges", self.edge_offsets)
        out = {k: getattr(self, k)[sl] for k in EDGE_FIELDS}
        out["time"] = self.time_stamps(out["edge_pos"])
        return out

    def _variables(self):
        data = super()._variables()
        data.update({k: (("edge",), getattr(self, k)) for k in EDGE_FIELDS})
        data["edge_offsets"] = (("track_edge",), self.edge_offsets)
        return data


def mhw_track_genealogy(mhw, obj, ids=None, neighbours=None, _compute=None):
    """The daily split and merge graph of the objects of mhw_objects(): the links between the connected parts of
    consecutive days, and per day how many parts were born, merged, ended and split.

    ``mhw``, ``obj``, ``ids`` and ``neighbours`` mean and validate what they do in mhw_track_parts(); give the same
    ``ids`` and the result lines up with its TrackPartsDataset and with the TrackDataset of mhw_tracks() entry for entry.

    Returns a TrackGenealogyDataset (module docstring: the definition and the identities; class docstring: the fields).
    Every number is an integer count and the edges are sorted: exact, and the same from run to run.  ``_compute``: a
    stand-in for track_genealogy_device() (host tests)."""
    sel = Selection(mhw, obj, ids, "mhw_track_genealogy")
    K = sel.neighbours_k(neighbours)
    axis = sel.periodic_axis()
    sshape, m = sel.sshape, sel.m
    sel.view()
    cell_index = sel.cell_index
    if (np.diff(cell_index) <= 0).any():               # the smallest compact cell of a part is then its smallest grid index
        raise XmhwException("mhw.cell_index should ascend, as detect() returns it")
    sel.layout()
    L, t0, offsets = sel.L, sel.time_start, sel.offsets
    vox_off = voxel_offsets(sel.start, sel.end, sel.slot)     # refuses V >= 2**31: nothing of size L or V exists yet
    V = int(vox_off[-1])
    if L == 0:
        got = sel.no_entries(dict.fromkeys(STAGE_FIELDS, np.int32))
    else:
        nbr = neighbour_table(cell_index, sshape, 6 if K == 4 else 26, axis)
        got = (_compute or track_genealogy_device)(sel.start, sel.end, sel.slot, sel.cell_of_row, sel.row_offsets, nbr,
                                                   vox_off, t0, offsets)
    edges = {k: np.ascontiguousarray(got[k], dtype=np.int32) for k in EDGE_FIELDS}
    f = dict(sel.stage_arrays(got, dict.fromkeys(COUNT_FIELDS, np.int32), "track genealogy"), **edges)
    E = f["edge_track"].shape[0]
    if any(f[k].shape != (E,) for k in EDGE_FIELDS):
        raise XmhwException("track genealogy stage returned edge arrays of different lengths")
    if L and f["n_parts"].min() < 1:
        raise XmhwException(f"{int((f['n_parts'] < 1).sum())} days of the selected objects hold no cell: obj does not belong "
                            "to mhw")
    C = cell_index.shape[0]
    if E and (f["edge_track"].min() < 0 or f["edge_track"].max() >= m or min(f["edge_from"].min(), f["edge_to"].min()) < 0 or
              max(f["edge_from"].max(), f["edge_to"].max()) >= C):
        raise XmhwException("track genealogy stage returned edges outside the selection or the cells")
    cell_index = np.asarray(cell_index, dtype=np.int64)
    track, pos, a, b = sort_edges(f["edge_track"], f["edge_pos"], cell_index[f["edge_from"]], cell_index[f["edge_to"]])
    first = offsets[:-1]
    entry = offsets[track] + (pos.astype(np.int64) - t0[track])
    # an edge belongs to the entry of its later day: never the first day of its object
    if (entry <= first[track]).any() or (entry >= offsets[1:][track]).any() or \
            (np.bincount(entry, minlength=L) != f["n_links"]).any():
        raise XmhwException("track genealogy stage returned edges that do not fit its n_links")
    f.update(edge_track=track, edge_pos=pos, edge_from=a, edge_to=b)
    f["edge_offsets"] = np.concatenate([[0], np.cumsum(np.bincount(track, minlength=m))]).astype(np.int64)
    f.update(sel.common_fields(), pos=sel.pos())
    if m:
        total = {k: np.add.reduceat(f[k].astype(np.int64), first) for k in ("n_parts", "n_born", "n_merged", "n_ended", "n_split")}
        f["n_splits"], f["n_merges"], f["n_nodes"] = total["n_split"], total["n_merged"], total["n_parts"]
        f["n_births"] = total["n_born"] - f["n_born"][first]
        f["n_ends"] = total["n_ended"] - f["n_ended"][offsets[1:] - 1]
        f["n_edges"] = np.diff(f["edge_offsets"])
    else:
        for k in ("n_splits", "n_merges", "n_nodes", "n_births", "n_ends", "n_edges"):
            f[k] = np.zeros(0, dtype=np.int64)
    return TrackGenealogyDataset(f, mhw.time, mhw.sdims, sshape, K, obj.periodic, V)
