"""mhw_objects(): the per-cell events of detect() grouped into objects connected in space and time -- "the
2013-2016 Pacific blob" as one thing instead of a hundred thousand table rows.  Not in xmhw nor in
marineHeatWaves; the tracking tools of the field (Ocetrac and its relatives) label a dense (time, lat, lon)
boolean volume on the CPU.  Here the volume is never built: the event table is an exact run-length encoding
of it, and its connected components are those of a graph on the table rows.

Voxels.  Row r of ``mhw.table``, in ocean cell c, occupies the time positions index_start[r]..index_end[r]
(inclusive; gap days of joined events included -- the `event` state of mhw_coverage()) of the grid point
``mhw.cell_index[c]`` of the stacked grid ``mhw.sshape``.  Land holds no voxel.
Neighbours.  connectivity=6: the same cell on consecutive days, or the same day in cells one step apart along
exactly one spatial dim.  connectivity=26: |dt| <= 1, |di| <= 1, |dj| <= 1, not all zero.  ``periodic`` names
one spatial dim that wraps.  An object is a connected component of the voxels.

The event graph.  Rows a, b are linked iff their cells are different spatial neighbours (4 or 8) and
start_a <= end_b + g and start_b <= end_a + g, g = 0 for 6 and 1 for 26.  The voxels of a row are connected
among themselves (consecutive days of one cell); two rows of one cell are at least a day apart, so no voxel
edge joins them directly (checked here); a voxel edge between two cells exists iff two of their rows come
within g days of each other.  Hence the components of the graph are the components of the voxels.

Host side here (validation, neighbour table, column slicing, weights, numbering); device side in
csrc/kernels_objects.hip.
"""
import numpy as np

from ._lib import hip
from .detect import EventDataset
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .gridweights import quantise_weights, resolve_weights, weights_label

PER_OBJECT = ("n_events", "n_cells", "time_start", "time_end", "cell_days", "area_days_q", "intensity_max", "peak_row")
_DTYPES = dict(n_events=np.int32, n_cells=np.int32, time_start=np.int32, time_end=np.int32, cell_days=np.int64,
               area_days_q=np.int64, intensity_max=np.float64, peak_row=np.int32)
_DIAGONAL = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def neighbour_table(cell_index, sshape, connectivity=6, periodic_axis=None):
    """nbr (C, 4 | 8) int32: the compact cell number of every spatial neighbour of every ocean cell, -1 for
    land, outside the grid, or the cell itself (a wrapping dim of length 1 or 2 folds neighbours together)."""
    ny, nx = (int(v) for v in sshape)
    cell_index = np.asarray(cell_index, dtype=np.int64)
    C = cell_index.shape[0]
    steps = _DIAGONAL[:4] if connectivity == 6 else _DIAGONAL
    number = np.full(ny * nx, -1, dtype=np.int32)
    number[cell_index] = np.arange(C, dtype=np.int32)
    i, j = np.divmod(cell_index, nx)
    nbr = np.full((C, len(steps)), -1, dtype=np.int32)
    own = np.arange(C, dtype=np.int32)
    for k, (di, dj) in enumerate(steps):
        ii, jj = i + di, j + dj
        if periodic_axis == 0:
            ii %= ny
        if periodic_axis == 1:
            jj %= nx
        ok = (ii >= 0) & (ii < ny) & (jj >= 0) & (jj < nx)
        v = np.full(C, -1, dtype=np.int32)
        v[ok] = number[ii[ok] * nx + jj[ok]]
        v[v == own] = -1
        nbr[:, k] = v
    return nbr


def weight_bits(total_days):
    """Bits of the quantised weights: 31, or fewer where sum(wq * duration) <= 2**bits * total_days could pass int64."""
    return int(min(31, 62 - int(total_days).bit_length()))


def objects_device(start, end, imax, offsets, nbr, gap, wq):
    """The device stage on compact arrays: start / end (n,) int32 positions of every table row, imax (n,)
    float64, offsets (C+1,), nbr (C, K) int32, gap 0 | 1, wq (C,) int64.  Returns a dict: ``root`` (n,) int32,
    the smallest row of every row's object, and the PER_OBJECT arrays, one entry per object in ascending root
    order."""
    h = hip()
    start = np.ascontiguousarray(start, dtype=np.int32)
    end = np.ascontiguousarray(end, dtype=np.int32)
    imax = np.ascontiguousarray(imax, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    wq = np.ascontiguousarray(wq, dtype=np.int64)
    n, C = start.shape[0], offsets.shape[0] - 1
    if n >= 1 << 31:
        raise XmhwException(f"mhw_objects handles fewer than 2**31 events, got {n}")
    if n == 0:
        return dict(root=np.zeros(0, dtype=np.int32), **{k: np.zeros(0, dtype=_DTYPES[k]) for k in PER_OBJECT})
    with DeviceScope() as s:
        with as_xmhw_errors(also="Unsupported"):
            d_start, d_end, d_off, d_nbr = s.upload(start), s.upload(end), s.upload(offsets), s.upload(nbr)
            d_cell, d_root = s.alloc(4 * n), s.alloc(4 * n)
            h.event_objects(d_start.ptr, d_end.ptr, n, d_off.ptr, C, d_nbr.ptr, nbr.shape[1], int(gap), d_cell.ptr, d_root.ptr)
            h.stream_sync(0)
            root = d_root.to_array((n,), np.int32)
            # slots in ascending root order: a root is its own root
            roots = np.nonzero(root == np.arange(n, dtype=np.int32))[0]
            m = roots.shape[0]
            slot_of_root = np.empty(n, dtype=np.int32)
            slot_of_root[roots] = np.arange(m, dtype=np.int32)
            d_slot = s.upload(slot_of_root[root])
            d_imax, d_wq = s.upload(imax), s.upload(wq)
            outs = {k: s.alloc(np.dtype(_DTYPES[k]).itemsize * m) for k in PER_OBJECT}
            h.object_reduce(d_start.ptr, d_end.ptr, d_imax.ptr, n, d_cell.ptr, d_off.ptr, d_wq.ptr, d_slot.ptr, m,
                            *[outs[k].ptr for k in PER_OBJECT])
            h.stream_sync(0)
        return dict(root=root, **{k: outs[k].to_array((m,), _DTYPES[k]) for k in PER_OBJECT})


class ObjectDataset:
    """What mhw_objects() returns, as plain arrays.  Objects are numbered 0..n_objects-1 in ascending
    (time_start, root) order.

    object (n_events,) int32        the object of every row of ``mhw.table``;
    root (n_objects,) int32         the smallest table row of each object;
    n_events, n_cells               rows and distinct cells of each object;
    time_start, time_end, duration  min index_start, max index_end (positions along ``time``), their span in steps;
    cell_days int64                 the sum of the event durations (voxels);
    area_days_q int64               the sum of wq[cell] * duration: ``area_days_q * weight_unit`` is an area x time
                                    in the units of the weights (``weight_unit = w.max() / 2**weight_bits``);
    intensity_max, peak_row         the largest intensity_max of the object's rows (NaN rows ignored; NaN if all
                                    are; -0.0 counts as 0.0) and the smallest row attaining it (-1 for NaN);
    time_peak, peak_cell            that row's time_peak position (NaN) and flat grid index (-1)."""

    def __init__(self, fields, time, sdims, sshape, coords, row_start, row_end, row_flat, weight_bits, weight_unit,
                 connectivity, periodic, attrs=None):
        for k, v in fields.items():
            setattr(self, k, v)
        self.time, self.sdims, self.sshape, self.coords = np.asarray(time), tuple(sdims), tuple(sshape), coords
        self._start, self._end, self._flat = row_start, row_end, row_flat
        self.weight_bits, self.weight_unit = int(weight_bits), float(weight_unit)
        self.connectivity, self.periodic = connectivity, periodic
        self.attrs = dict(attrs or {})

    @property
    def n_objects(self):
        return int(self.root.shape[0])

    time_stamps = EventDataset.time_stamps

    def label_map(self, pos):
        """The ``sshape`` int32 map of the object ids present on time position ``pos``, -1 elsewhere."""
        pos = int(pos)
        on = (self._start <= pos) & (self._end >= pos)
        out = np.full(int(np.prod(self.sshape, dtype=np.int64)), -1, dtype=np.int32)
        out[self._flat[on]] = self.object[on]
        return out.reshape(self.sshape)

    def to_xarray(self):
        import xarray as xr
        per = {k: (("object",), getattr(self, k)) for k in ("root", "n_events", "n_cells", "duration", "cell_days",
                                                           "area_days_q", "intensity_max", "peak_row", "peak_cell")}
        for k in ("time_start", "time_end", "time_peak"):
            per[k] = (("object",), self.time_stamps(getattr(self, k)))
        per["object_of_event"] = (("event",), self.object)
        return xr.Dataset(per, coords={"object": np.arange(self.n_objects)},
                          attrs=dict(self.attrs, weight_unit=self.weight_unit, weight_bits=self.weight_bits,
                                     connectivity=self.connectivity, periodic=self.periodic or ""))


def mhw_objects(mhw, connectivity=6, periodic=None, weights=None, _compute=None):
    """Group the events of a gridded detect() into objects connected in space and time.

    ``mhw``: the EventDataset returned by detect() on a grid with two spatial dims.  ``connectivity``: 6 (faces:
    the same day in cells one step apart along one dim) or 26 (faces, edges and corners, a day apart included).
    ``periodic``: the name of one spatial dim that wraps (longitude on a global grid), or None.  ``weights``: None
    (1 per cell), "coslat" or an array on the spatial grid (dims ``mhw.sdims``), as for mhw_coverage(); they are
    quantised to ``rint(w / w.max() * 2**weight_bits)``, weight_bits = min(31, 62 - bit_length(sum of all
    durations)), and summed as integers.

    Returns an ObjectDataset.  Every number in it is an integer, a minimum or a maximum: exact, and independent
    of launch geometry and scheduling.  ``_compute``: a stand-in for objects_device() (host tests)."""
    if not isinstance(mhw, EventDataset):
        raise XmhwException("mhw_objects expects the EventDataset returned by xmhw_amd.detect()")
    if mhw.point:
        raise XmhwException("mhw_objects needs a grid: a single-point series has no neighbours")
    if len(mhw.sdims) != 2:
        raise XmhwException(f"mhw_objects handles two spatial dims, got {mhw.sdims}")
    if connectivity not in (6, 26):
        raise XmhwException(f"connectivity should be 6 or 26, got {connectivity!r}")
    if periodic is not None and periodic not in mhw.sdims:
        raise XmhwException(f"periodic should be None or one of {mhw.sdims}, got {periodic!r}")
    sshape = tuple(int(v) for v in mhw.sshape)
    w = resolve_weights(weights, mhw.coords, list(mhw.sdims), None, list(mhw.sdims), sshape)
    n = mhw.n_events
    if n >= 1 << 31:
        raise XmhwException(f"mhw_objects handles fewer than 2**31 events, got {n}")
    view = mhw.compact_view()
    offsets, cell_index, cell_of_row, start, end = (view[k] for k in ("offsets", "cell_index", "cell_of_row", "start", "end"))
    cols = mhw.columns
    imax = np.ascontiguousarray(mhw.table[:, cols.index("intensity_max")], dtype=np.float64)
    same = cell_of_row[1:] == cell_of_row[:-1]
    if (start[1:][same].astype(np.int64) <= end[:-1][same].astype(np.int64) + 1).any():
        raise XmhwException("events of one cell should be in time order and at least one step apart")
    total_days = int((end.astype(np.int64) - start + 1).sum())
    bits = weight_bits(total_days)
    wq, unit = quantise_weights(w, bits)
    nbr = neighbour_table(cell_index, sshape, connectivity, None if periodic is None else mhw.sdims.index(periodic))
    compute = _compute or objects_device
    got = compute(start, end, imax, offsets, nbr, 0 if connectivity == 6 else 1, wq[cell_index])
    root_of_row = np.asarray(got["root"], dtype=np.int32)
    if root_of_row.shape != (n,) or (n and not ((root_of_row >= 0) & (root_of_row <= np.arange(n))).all()):
        raise XmhwException("objects stage returned roots that are not rows at or before their own")
    roots = np.nonzero(root_of_row == np.arange(n, dtype=np.int32))[0].astype(np.int32)     # a root is its own root
    m = roots.shape[0]
    slot_of_root = np.full(n, -1, dtype=np.int32)
    slot_of_root[roots] = np.arange(m, dtype=np.int32)
    slot_of_row = slot_of_root[root_of_row]
    if n and slot_of_row.min() < 0:
        raise XmhwException("objects stage returned a root that is not its own root")
    per = {k: np.asarray(got[k], dtype=_DTYPES[k]) for k in PER_OBJECT}
    if any(v.shape != (m,) for v in per.values()):
        raise XmhwException(f"objects stage returned arrays that do not fit {n} events in {m} objects")
    # object ids in ascending (time_start, root) order
    order = np.argsort(per["time_start"], kind="stable")          # roots are ascending already
    new_id = np.empty(m, dtype=np.int32)
    new_id[order] = np.arange(m, dtype=np.int32)
    fields = {k: np.ascontiguousarray(v[order]) for k, v in per.items()}
    fields["root"] = roots[order]
    fields["object"] = new_id[slot_of_row]
    fields["duration"] = fields["time_end"] - fields["time_start"] + 1
    pk = fields["peak_row"]
    has = pk >= 0
    tp = np.full(m, np.nan)
    tp[has] = mhw.table[pk[has], cols.index("time_peak")]
    pc = np.full(m, -1, dtype=np.int64)
    pc[has] = cell_index[cell_of_row[pk[has]]]
    fields["time_peak"], fields["peak_cell"] = tp, pc
    attrs = {"weights": weights_label(weights)}
    if "xmhw_parameters" in mhw.attrs:
        attrs["xmhw_parameters"] = mhw.attrs["xmhw_parameters"]
    return ObjectDataset(fields, mhw.time, mhw.sdims, sshape, mhw.coords, start, end, cell_index[cell_of_row], bits, unit,
                         connectivity, periodic, attrs)
