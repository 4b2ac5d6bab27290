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

from ._lib import hip
from .detect import EventDataset
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .objects import neighbour_table
from .track_parts import voxel_offsets
from .tracks import checked_selection, selection_layout

COUNT_FIELDS = ("n_parts", "n_links", "n_born", "n_merged", "n_ended", "n_split")       # XMHW_GENEALOGY_* order
EDGE_FIELDS = ("edge_track", "edge_pos", "edge_from", "edge_to")
STAGE_FIELDS = COUNT_FIELDS + EDGE_FIELDS
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
    start = np.ascontiguousarray(start, dtype=np.int32)
    end = np.ascontiguousarray(end, dtype=np.int32)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    cell = np.ascontiguousarray(cell, dtype=np.int32)
    row_offsets = np.ascontiguousarray(row_offsets, dtype=np.int64)
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    vox_off = np.ascontiguousarray(vox_off, dtype=np.int64)
    time_start = np.ascontiguousarray(time_start, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n, m = start.shape[0], time_start.shape[0]
    L = int(offsets[-1])
    if L == 0 or n == 0 or m == 0:
        return {k: np.zeros(L if k in COUNT_FIELDS else 0, dtype=np.int32) for k in STAGE_FIELDS}
    C = row_offsets.shape[0] - 1
    if nbr.ndim != 2 or nbr.shape[0] != C or cell.shape != (n,) or vox_off.shape != (n + 1,):
        raise XmhwException("the neighbour table, the row offsets and the voxel offsets do not fit the rows and cells")
    V = int(vox_off[-1])
    cap = edge_capacity(start, end, slot, cell)
    if max(n, m, L, V, C, cap) >= 1 << 31:
        raise XmhwException(f"mhw_track_genealogy handles fewer than 2**31 rows, objects, series entries and voxels, got {n}, "
                            f"{m}, {L}, {V}: select fewer objects with ids=")
    h = hip()
    F = len(COUNT_FIELDS)
    with DeviceScope() as s:
        with as_xmhw_errors(also="Unsupported", hint="select fewer objects with ids="):
            d = [s.upload(a) for a in (start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets)]
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


class TrackGenealogyDataset:
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

    def __init__(self, fields, time, sdims, sshape, neighbours, periodic, n_voxels, attrs=None):
        for k, v in fields.items():
            setattr(self, k, v)
        self.time, self.sdims, self.sshape = np.asarray(time), tuple(sdims), tuple(sshape)
        self.neighbours, self.periodic, self.n_voxels = int(neighbours), periodic, int(n_voxels)
        self.attrs = dict(attrs or {})

    @property
    def n_selected(self):
        return int(self.ids.shape[0])

    time_stamps = EventDataset.time_stamps

    def _position(self, i, who):
        i = int(i)
        if not 0 <= i < self.n_selected:
            raise XmhwException(f"{who}() takes a position in [0, {self.n_selected}), got {i}")
        return i

    def series(self, i):
        """The slices of the i-th selected object: a dict of its series plus ``time``, the stamps of its days."""
        i = self._position(i, "series")
        sl = slice(int(self.offsets[i]), int(self.offsets[i + 1]))
        out = {k: getattr(self, k)[sl] for k in self._SERIES}
        out["time"] = self.time_stamps(out["pos"])
        return out

    def edges(self, i):
        """The edges of the i-th selected object: a dict of its slices of the four edge arrays plus ``time``, the stamps
        of the later days."""
        i = self._position(i, "edges")
        sl = slice(int(self.edge_offsets[i]), int(self.edge_offsets[i + 1]))
        out = {k: getattr(self, k)[sl] for k in EDGE_FIELDS}
        out["time"] = self.time_stamps(out["edge_pos"])
        return out

    def to_xarray(self):
        import xarray as xr
        data = {k: (("obs",), getattr(self, k)) for k in self._SERIES}
        data["time"] = (("obs",), self.time_stamps(self.pos))
        for k in EDGE_FIELDS:
            data[k] = (("edge",), getattr(self, k))
        for k in self._PER_OBJECT:
            data["object_id" if k == "ids" else k] = (("track",), getattr(self, k))
        data["offsets"] = (("track_edge",), self.offsets)
        data["edge_offsets"] = (("track_edge",), self.edge_offsets)
        return xr.Dataset(data, attrs=dict(self.attrs, neighbours=self.neighbours, periodic=self.periodic or ""))


def mhw_track_genealogy(mhw, obj, ids=None, neighbours=None, _compute=None):
    """The daily split and merge graph of the objects of mhw_objects(): the links between the connected parts of
    consecutive days, and per day how many parts were born, merged, ended and split.

    ``mhw``, ``obj``, ``ids`` and ``neighbours`` mean and validate what they do in mhw_track_parts(); give the same
    ``ids`` and the result lines up with its TrackPartsDataset and with the TrackDataset of mhw_tracks() entry for entry.

    Returns a TrackGenealogyDataset (module docstring: the definition and the identities; class docstring: the fields).
    Every number is an integer count and the edges are sorted: exact, and the same from run to run.  ``_compute``: a
    stand-in for track_genealogy_device() (host tests)."""
    sshape, object_of_row, ids = checked_selection(mhw, obj, ids, "mhw_track_genealogy")
    if neighbours not in (None, 4, 8):
        raise XmhwException(f"neighbours should be None, 4 or 8, got {neighbours!r}")
    if obj.connectivity not in (6, 26):
        raise XmhwException(f"obj.connectivity should be 6 or 26, got {obj.connectivity!r}")
    if obj.periodic is not None and obj.periodic not in mhw.sdims:
        raise XmhwException(f"obj.periodic should be None or one of {mhw.sdims}, got {obj.periodic!r}: obj does not belong "
                            "to mhw")
    K = int(neighbours) if neighbours is not None else (4 if obj.connectivity == 6 else 8)
    m = ids.shape[0]
    view = mhw.compact_view()
    cell_index, start, end = (view[k] for k in ("cell_index", "start", "end"))
    if (np.diff(cell_index) <= 0).any():               # the smallest compact cell of a part is then its smallest grid index
        raise XmhwException("mhw.cell_index should ascend, as detect() returns it")
    t0, t1, dur, offsets, slot = selection_layout(obj, ids, object_of_row, start, end)
    L = int(offsets[-1])
    vox_off = voxel_offsets(start, end, slot)          # refuses V >= 2**31: nothing of size L or V exists yet
    V = int(vox_off[-1])
    if L == 0:
        got = {k: np.zeros(0, dtype=np.int32) for k in STAGE_FIELDS}
    else:
        axis = None if obj.periodic is None else mhw.sdims.index(obj.periodic)
        nbr = neighbour_table(cell_index, sshape, 6 if K == 4 else 26, axis)
        got = (_compute or track_genealogy_device)(start, end, slot, view["cell_of_row"].astype(np.int32), view["offsets"], nbr,
                                                   vox_off, t0, offsets)
    f = {k: np.ascontiguousarray(got[k], dtype=np.int32) for k in STAGE_FIELDS}
    if any(f[k].shape != (L,) for k in COUNT_FIELDS):
        raise XmhwException(f"track genealogy stage returned arrays that do not fit {L} entries")
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
    f.update(ids=ids, offsets=offsets, time_start=t0, time_end=t1, duration=dur.astype(np.int32))
    f["pos"] = (np.arange(L, dtype=np.int64) - np.repeat(first - t0, dur)).astype(np.int32)
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
