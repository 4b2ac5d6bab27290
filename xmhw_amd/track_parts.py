"""mhw_track_parts(): into how many connected parts every object of mhw_objects() falls on each of its days, aligned
entry for entry with the ragged (CSR) arrays of mhw_tracks(): entry offsets[i] + (t - time_start[i]) belongs to object
ids[i] on time position t.  Objects chain through time, so one object is often several separate patches that touched
once; its daily area and its centre (a vector mean of disjoint patches) mean little unless the user knows it.  The
tracking tools of the field label every day of a dense volume; here the volume is never built: the voxels of the
selected rows are numbered, and the lock-free union-find of mhw_objects() runs on them one day at a time
(csrc/kernels_parts.hip).

The definition.  Take a selected object o and a time position t in [time_start[o], time_end[o]].
  * Its footprint is the set of ocean cells that hold a table row of o covering t (index_start..index_end inclusive,
    gap days of joined events included: the voxels of objects.py).
  * Two footprint cells are adjacent iff they are spatial neighbours in neighbour_table(cell_index, sshape, K,
    periodic_axis), K = 6 (4 neighbours: one step along exactly one spatial dim) or 26 (8 neighbours: the diagonals
    too).  ``neighbours=None`` takes obj.connectivity; ``neighbours=4 | 8`` overrides it.  The wrapping axis is always
    obj.periodic.
  * A part is a connected component of the footprint under that adjacency.
  * Parts never join cells of different objects: with neighbours=8 on objects built with connectivity 6 two diagonal
    cells may belong to different objects, and each stays in its own object's footprint.  The device therefore unites
    only rows of equal slot.
Per entry, exact integers:
    n_parts (int32)         the number of parts,
    cells_largest (int32)   the most cells in one part,
    area_largest_q (int64)  the largest sum of wq[c] over one part, wq = rint(w / w.max() * 2**obj.weight_bits), the
                            quantisation of mhw_tracks().
The two maxima are independent: the part with the most cells need not be the part with the largest area.

Identities, against mhw_tracks() on the same ids and weights:
    n_parts >= 1 on every entry (an object is connected in space and time: it has no empty day);
    n_parts + cells_largest - 1 <= n_cells (every other part holds at least one cell);
    where n_parts == 1: cells_largest == n_cells and area_largest_q == area_q.

Derived on the host, per selected object: n_parts_max and pos_n_parts_max (the first position that attains it),
days_split (the entries with n_parts > 1); per entry area_largest = area_largest_q * weight_unit.

Voxels.  Only rows of selected objects have voxels.  vox_off is the (n + 1,) exclusive prefix sum of the durations of
the selected rows (an unselected row counts 0), V = vox_off[-1], and day t of row r is voxel vox_off[r] + t - start[r].
The device keeps 16 bytes per voxel; V >= 2**31 is refused before anything is allocated.

The genealogy -- which part of day t continues into which part of day t + 1, and the split and merge counts taken from
it -- is mhw_track_genealogy() (track_genealogy.py), on the same voxels and the same union-find.

Host side here (validation, selection, neighbour table, weights, voxel numbering, the derived fields); device side in
csrc/kernels_parts.hip behind track_parts_device().
"""
import numpy as np

from .exception import XmhwException
from .gridweights import quantise_weights, resolve_weights, weights_label
from .objects import neighbour_table
from .track_common import ChainDataset, Selection, device_stage, stage_inputs

STAGE_FIELDS = ("n_parts", "cells_largest", "area_largest_q")
_DTYPES = dict(n_parts=np.int32, cells_largest=np.int32, area_largest_q=np.int64)
_INPUTS = dict(start=np.int32, end=np.int32, slot=np.int32, cell=np.int32, row_offsets=np.int64, nbr=np.int32, wq=np.int64,
               vox_off=np.int64, time_start=np.int32, offsets=np.int64)
VOXEL_BYTES = 16                # XMHW_PARTS_VOXEL_BYTES (include/xmhw_amd.h)


def voxel_offsets(start, end, slot):
    """vox_off (n + 1,) int64 of the module docstring for rows start..end (inclusive) with ``slot`` >= 0 where selected.
    Raises where V = vox_off[-1] reaches 2**31; touches nothing but the three arrays."""
    days = np.where(np.asarray(slot) >= 0, np.asarray(end, dtype=np.int64) - np.asarray(start, dtype=np.int64) + 1, 0)
    if days.size and days.min() < 0:
        raise XmhwException("a table row ends before it starts")
    vox_off = np.concatenate([[0], np.cumsum(days, dtype=np.int64)]).astype(np.int64)
    V = int(vox_off[-1])
    if V >= 1 << 31:
        raise XmhwException(f"the selected objects hold {V} voxels (days of table rows), 2**31 and more, at {VOXEL_BYTES} "
                            "bytes each on the device: select fewer objects with ids=")
    return vox_off


def track_parts_device(start, end, slot, cell, row_offsets, nbr, wq, vox_off, time_start, offsets):
    """The device stage.  start / end (n,) int32 positions of every table row; slot (n,) int32, the position of the row's
    object in the selection or -1; cell (n,) int32, the row's compact cell; row_offsets (C + 1,) int64, the rows of every
    cell; nbr (C, K) int32; wq (C,) int64; vox_off (n + 1,) int64 (voxel_offsets()); time_start (m,) int32 and offsets
    (m + 1,) int64 of the selection.  Returns a dict of STAGE_FIELDS, (L,) each, L = offsets[-1]."""
    start, end, slot, cell, row_offsets, nbr, wq, vox_off, time_start, offsets = a = stage_inputs(
        _INPUTS, start, end, slot, cell, row_offsets, nbr, wq, vox_off, time_start, offsets)
    n, m, C = start.shape[0], time_start.shape[0], wq.shape[0]
    L = int(offsets[-1])
    if L == 0 or n == 0 or m == 0:
        return {k: np.zeros(L, dtype=_DTYPES[k]) for k in STAGE_FIELDS}
    if nbr.ndim != 2 or nbr.shape[0] != C or row_offsets.shape != (C + 1,) or vox_off.shape != (n + 1,):
        raise XmhwException("the neighbour table, the row offsets and the voxel offsets do not fit the rows and cells")
    V = int(vox_off[-1])
    with device_stage(a, (n, m, L, V, C), f"mhw_track_parts handles fewer than 2**31 rows, objects, series entries and voxels, "
                      f"got {n}, {m}, {L}, {V}") as (h, s, d, launch):
        with launch:
            d_np, d_cl, d_al, d_bad = s.alloc(4 * L), s.alloc(4 * L), s.alloc(8 * L), s.alloc(4)
            h.object_parts(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, n, d[4].ptr, C, d[5].ptr, nbr.shape[1], d[6].ptr, d[7].ptr, V,
                           d[8].ptr, d[9].ptr, m, L, d_np.ptr, d_cl.ptr, d_al.ptr, d_bad.ptr)
            h.stream_sync(0)
        out = dict(n_parts=d_np.to_array((L,), np.int32), cells_largest=d_cl.to_array((L,), np.int32),
                   area_largest_q=d_al.to_array((L,), np.int64))
        bad = int(d_bad.to_array((1,), np.int32)[0])
    if bad:
        raise XmhwException(f"{bad} table rows do not lie within their object's days, cells or voxels: obj does not belong "
                            "to mhw")
    return out


class TrackPartsDataset(ChainDataset):
    """What mhw_track_parts() returns, as plain arrays, aligned with the TrackDataset of the same ``ids``: m objects, L =
    offsets[-1] entries; entry offsets[i] + (t - time_start[i]) belongs to object ids[i] on time position t.

    ids, offsets, time_start, time_end, duration, pos    as in the TrackDataset;
    n_parts (L,) int32              the connected parts of the object's footprint on that day (>= 1);
    cells_largest (L,) int32        the most cells in one part;
    area_largest_q (L,) int64, area_largest     the largest sum of quantised weights over one part, and
                                    ``area_largest_q * weight_unit`` (float64); an independent maximum: it may come
                                    from another part than cells_largest;
    n_parts_max (m,) int32          the largest n_parts of each object;
    pos_n_parts_max (m,) int32      the first time position that attains it;
    days_split (m,) int32           the object's days with n_parts > 1;
    neighbours 4 | 8, periodic, weight_bits, weight_unit, n_voxels (V)."""

    _SERIES = ("pos", "n_parts", "cells_largest", "area_largest_q", "area_largest")
    _PER_OBJECT = ("ids", "time_start", "time_end", "duration", "n_parts_max", "pos_n_parts_max", "days_split")
    _ATTRS = ("neighbours", "periodic", "weight_unit", "weight_bits")

    def __init__(self, fields, time, sdims, sshape, neighbours, periodic, weight_bits, weight_unit, n_voxels, attrs=None):
        super().__init__(fields, time, sdims, sshape, attrs)
        self.neighbours, self.periodic = int(neighbours), periodic
        self.weight_bits, self.weight_unit, self.n_voxels = int(weight_bits), float(weight_unit), int(n_voxels)


def mhw_track_parts(mhw, obj, ids=None, weights=None, neighbours=None, _compute=None):
    """The daily connected parts of the objects of mhw_objects(): how many, and how large the largest is.

    ``mhw``, ``obj``, ``ids`` and ``weights`` mean and validate what they do in mhw_tracks(); give the same ``ids`` and
    ``weights`` and the result lines up with its TrackDataset entry for entry.  ``neighbours``: None (4 for objects of
    connectivity 6, 8 for 26), or 4 or 8; the wrapping dim is ``obj.periodic``.

    Returns a TrackPartsDataset (module docstring: the definition and the identities; class docstring: the fields).
    Every number is an integer sum or maximum: exact, and the same from run to run.  ``_compute``: a stand-in for
    track_parts_device() (host tests)."""
    sel = Selection(mhw, obj, ids, "mhw_track_parts")
    K = sel.neighbours_k(neighbours)
    axis = sel.periodic_axis()
    sshape, sdims = sel.sshape, list(mhw.sdims)
    w = resolve_weights(weights, mhw.coords, sdims, None, sdims, sshape)
    sel.view()
    bits = obj.weight_bits
    wq, unit = quantise_weights(w, bits)
    sel.layout()
    L = sel.L
    vox_off = voxel_offsets(sel.start, sel.end, sel.slot)     # refuses V >= 2**31: nothing of size L or V exists yet
    V = int(vox_off[-1])
    if L == 0:
        got = sel.no_entries(_DTYPES)
    else:
        nbr = neighbour_table(sel.cell_index, sshape, 6 if K == 4 else 26, axis)
        got = (_compute or track_parts_device)(sel.start, sel.end, sel.slot, sel.cell_of_row, sel.row_offsets, nbr,
                                               wq[sel.cell_index], vox_off, sel.time_start, sel.offsets)
    f = sel.stage_arrays(got, _DTYPES, "track parts")
    if L and f["n_parts"].min() < 1:
        raise XmhwException(f"{int((f['n_parts'] < 1).sum())} days of the selected objects hold no cell: obj does not belong "
                            "to mhw")
    f.update(sel.common_fields(), pos=sel.pos())
    f["area_largest"] = f["area_largest_q"] * unit
    f["n_parts_max"], f["pos_n_parts_max"] = sel.first_max(f["n_parts"])
    f["days_split"] = sel.count_days(f["n_parts"] > 1)
    attrs = {"weights": weights_label(weights)}
    return TrackPartsDataset(f, mhw.time, mhw.sdims, sshape, K, obj.periodic, bits, unit, V, attrs)
