"""What the stages downstream of mhw_objects() share (mhw_tracks, mhw_track_intensity, mhw_track_parts,
mhw_track_genealogy, mhw_track_shape): the selection of objects with its ragged layout and the table
rows that fill it (Selection), the plain-array dataset every stage returns (ChainDataset), and the frame of their device
stages (stage_inputs, device_stage).  Object i of a selection owns the entries offsets[i]..offsets[i + 1] - 1 of every
series, one per time position from time_start[i] to time_end[i]."""
from contextlib import contextmanager

import numpy as np

from ._lib import hip
from .detect import EventDataset
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .objects import ObjectDataset


class ChainDataset:
    """The arrays of one stage for m selected objects and L = offsets[-1] entries.  A subclass names its per-entry fields
    in _SERIES, its per-object fields in _PER_OBJECT (a field that is None is left out everywhere) and the scalar
    attributes that to_xarray() records in _ATTRS, and adds what only it has."""

    _SERIES = _PER_OBJECT = _ATTRS = ()
    _COORDS = None                                   # to_xarray(): coordinates beside the variables

    def __init__(self, fields, time, sdims, sshape, attrs=None):
        for k, v in fields.items():
            setattr(self, k, v)
        self.time, self.sdims, self.sshape = np.asarray(time), tuple(sdims), tuple(sshape)
        self.attrs = dict(attrs or {})

    @property
    def n_selected(self):
        return int(self.ids.shape[0])

    time_stamps = EventDataset.time_stamps

    def _span(self, i, who="series", offsets=None):
        """the slice of the i-th selected object in the arrays laid out by ``offsets`` (default: the series)"""
        i = int(i)
        if not 0 <= i < self.n_selected:
            raise XmhwException(f"{who}() takes a position in [0, {self.n_selected}), got {i}")
        offsets = self.offsets if offsets is None else offsets
        return slice(int(offsets[i]), int(offsets[i + 1]))

    def series(self, i):
        """The slices of the i-th selected object: a dict of its series plus ``time``, the stamps of its days."""
        sl = self._span(i)
        out = {k: getattr(self, k)[sl] for k in self._SERIES if getattr(self, k) is not None}
        out["time"] = self.time_stamps(out["pos"])
        return out

    def _variables(self):
        """to_xarray(): name -> (dims, array)"""
        data = {k: (("obs",), getattr(self, k)) for k in self._SERIES if getattr(self, k) is not None}
        data["time"] = (("obs",), self.time_stamps(self.pos))
        for k in self._PER_OBJECT:
            if getattr(self, k) is not None:
                data["object_id" if k == "ids" else k] = (("track",), getattr(self, k))
        data["offsets"] = (("track_edge",), self.offsets)
        return data

    def to_xarray(self):
        import xarray as xr
        return xr.Dataset(self._variables(), coords=self._COORDS, attrs=dict(
            self.attrs, **{k: "" if getattr(self, k) is None else getattr(self, k) for k in self._ATTRS}))


def _slots(m_all, ids, object_of_row):
    """(n,) int32: the position of every row's object in ``ids``, -1 where it is not selected"""
    position = np.full(m_all, -1, dtype=np.int32)
    position[ids] = np.arange(ids.shape[0], dtype=np.int32)
    return position[object_of_row]


class Selection:
    """The selected objects of one call and the table rows that fill their series.  Selection(mhw, obj, ids, who) makes
    the checks every stage makes of its three arguments (``who``: the function's name in the messages) and holds sshape,
    ids (m,) int32 and m; view() adds the compact table, start / end (n,) int32, cell_of_row (n,) int32, row_offsets
    (C + 1,) int64, cell_index (C,) int64 and C; layout() adds time_start / time_end (m,) int32, duration (m,) int64,
    offsets (m + 1,) int64, L and slot (n,) int32.  The three are separate steps because each stage has refusals of its
    own that come between them."""

    def __init__(self, mhw, obj, ids, who):
        if not isinstance(mhw, EventDataset):
            raise XmhwException(f"{who} expects the EventDataset returned by xmhw_amd.detect()")
        if not isinstance(obj, ObjectDataset):
            raise XmhwException(f"{who} expects the ObjectDataset returned by xmhw_amd.mhw_objects()")
        if mhw.point:
            raise XmhwException(f"{who} needs a grid: a single-point series has no objects")
        if len(mhw.sdims) != 2:
            raise XmhwException(f"{who} handles two spatial dims, got {mhw.sdims}")
        n = mhw.n_events
        sshape = tuple(int(v) for v in mhw.sshape)
        if np.asarray(obj.object).shape != (n,) or tuple(obj.sshape) != sshape:
            raise XmhwException(f"obj.object should have one entry per table row ({n}) on the grid {sshape}: "
                                "obj does not belong to mhw")
        m_all = obj.n_objects
        object_of_row = np.asarray(obj.object, dtype=np.int64)
        if n and (object_of_row.min() < 0 or object_of_row.max() >= m_all):
            raise XmhwException("obj.object holds ids outside [0, n_objects)")
        if ids is None:
            ids = np.arange(m_all, dtype=np.int32)
        else:
            ids = np.asarray(ids)
            if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
                raise XmhwException("ids should be None or a 1-D integer array of object ids")
            ids = ids.astype(np.int64)
            if ids.size and (ids.min() < 0 or ids.max() >= m_all):
                raise XmhwException(f"ids should be in [0, {m_all})")
            if np.unique(ids).shape[0] != ids.shape[0]:
                raise XmhwException("ids should be distinct")
            ids = ids.astype(np.int32)
        self.mhw, self.obj, self.sshape, self.ids, self.m = mhw, obj, sshape, ids, ids.shape[0]
        self._object_of_row = object_of_row

    def view(self):
        v = self.mhw.compact_view()
        self.C, self.cell_index, self.start, self.end, self.row_offsets = (v[k] for k in ("C", "cell_index", "start", "end",
                                                                                          "offsets"))
        self.cell_of_row = v["cell_of_row"].astype(np.int32)

    def layout(self):
        if not hasattr(self, "start"):                 # the rows are what the layout is checked against
            self.view()
        obj, ids, m = self.obj, self.ids, self.m
        # the selection: where its objects start, how long they live, which rows are theirs
        t0 = np.ascontiguousarray(np.asarray(obj.time_start, dtype=np.int32)[ids])
        t1 = np.ascontiguousarray(np.asarray(obj.time_end, dtype=np.int32)[ids])
        dur = t1.astype(np.int64) - t0 + 1
        if m and dur.min() < 1:
            raise XmhwException("obj holds an object that ends before it starts")
        offsets = np.concatenate([[0], np.cumsum(dur)]).astype(np.int64)
        L = int(offsets[-1])
        if L + 1 >= 1 << 31:
            raise XmhwException(f"the series of the {m} selected objects hold {L} entries, 2**31 - 1 and more: select fewer "
                                "objects with ids=")
        slot = _slots(obj.n_objects, ids, self._object_of_row)
        sel = slot >= 0
        if sel.any() and ((self.start[sel] < t0[slot[sel]]).any() or (self.end[sel] > t1[slot[sel]]).any()):
            raise XmhwException("a table row lies outside the days of its object: obj does not belong to mhw")
        self.time_start, self.time_end, self.duration, self.offsets, self.L, self.slot = t0, t1, dur, offsets, L, slot

    @classmethod
    def of_tracks(cls, mhw, obj, tr, who):
        """The selection of the TrackDataset ``tr`` with its layout, checked against ``obj``: view() and layout() done."""
        self = cls.__new__(cls)
        n = mhw.n_events
        object_of_row = np.asarray(obj.object, dtype=np.int64)
        m_all = obj.n_objects
        if object_of_row.shape != (n,) or (n and (object_of_row.min() < 0 or object_of_row.max() >= m_all)):
            raise XmhwException("obj.object should hold one object id per table row: obj does not belong to mhw")
        ids = np.asarray(tr.ids, dtype=np.int64)
        m = ids.shape[0]
        if m and (ids.min() < 0 or ids.max() >= m_all or np.unique(ids).shape[0] != m):
            raise XmhwException("tr.ids should be distinct object ids of obj: tr does not belong to obj")
        t0 = np.ascontiguousarray(tr.time_start, dtype=np.int32)
        offsets = np.ascontiguousarray(tr.offsets, dtype=np.int64)
        dur = np.asarray(obj.time_end, dtype=np.int64)[ids] - np.asarray(obj.time_start, dtype=np.int64)[ids] + 1
        if (offsets.shape != (m + 1,) or not np.array_equal(t0, np.asarray(obj.time_start)[ids])
                or not np.array_equal(np.diff(offsets), dur) or offsets[0] != 0):
            raise XmhwException("tr.time_start and tr.offsets are not those of its objects in obj: tr does not belong to obj")
        L = int(offsets[-1])
        if L >= 1 << 31:
            raise XmhwException(f"the series of the {m} selected objects hold {L} entries, 2**31 and more: select fewer "
                                "objects with ids= in mhw_tracks()")
        self.mhw, self.obj, self.sshape, self.ids, self.m = mhw, obj, tuple(int(v) for v in mhw.sshape), tr.ids, m
        self.view()
        self.time_start, self.time_end, self.duration, self.offsets, self.L = t0, tr.time_end, dur, offsets, L
        self.slot = _slots(m_all, ids, object_of_row)
        if max(n, m, L) >= 1 << 31:
            raise XmhwException(f"{who} handles fewer than 2**31 rows, objects and series entries, got {n}, {m}, {L}: select "
                                "fewer objects with ids= in mhw_tracks()")
        return self

    def periodic_axis(self):
        """the axis of obj.periodic among the spatial dims, or None"""
        periodic, sdims = self.obj.periodic, self.mhw.sdims
        if periodic is not None and periodic not in sdims:
            raise XmhwException(f"obj.periodic should be None or one of {sdims}, got {periodic!r}: obj does not belong to mhw")
        return None if periodic is None else sdims.index(periodic)

    def neighbours_k(self, neighbours):
        """K of ``neighbours`` = None | 4 | 8: None takes 4 for objects of connectivity 6, 8 for 26"""
        if neighbours not in (None, 4, 8):
            raise XmhwException(f"neighbours should be None, 4 or 8, got {neighbours!r}")
        if self.obj.connectivity not in (6, 26):
            raise XmhwException(f"obj.connectivity should be 6 or 26, got {self.obj.connectivity!r}")
        return int(neighbours) if neighbours is not None else (4 if self.obj.connectivity == 6 else 8)

    def pos(self):
        """(L,) int32: the time position of every entry"""
        first = self.offsets[:-1]
        return (np.arange(self.L, dtype=np.int64) - np.repeat(first - self.time_start, np.diff(self.offsets))).astype(np.int32)

    def common_fields(self):
        return dict(ids=self.ids, offsets=self.offsets, time_start=self.time_start, time_end=self.time_end,
                    duration=self.duration.astype(np.int32))

    def first_max(self, values):
        """Per object: (the largest of its ``values`` (L,), the first time position that attains it as int32)"""
        if not self.m:
            return np.zeros(0, dtype=values.dtype), np.zeros(0, dtype=np.int32)
        first, L = self.offsets[:-1], self.L
        top = np.maximum.reduceat(values, first)
        at = np.where(values == np.repeat(top, np.diff(self.offsets)), np.arange(L, dtype=np.int64), L)
        return top, (np.minimum.reduceat(at, first) - first + self.time_start).astype(np.int32)

    def count_days(self, mask):
        """(m,) int32: the entries of every object on which ``mask`` (L,) holds"""
        if not self.m:
            return np.zeros(0, dtype=np.int32)
        return np.add.reduceat(mask.astype(np.int32), self.offsets[:-1]).astype(np.int32)

    def no_entries(self, spec):
        """what a stage returns for a selection without entries; ``spec`` as for stage_arrays()"""
        return {k: np.zeros(_lead(v) + (0,), dtype=_dtype(v)) for k, v in spec.items()}

    def stage_arrays(self, got, spec, who):
        """The arrays a device stage (or its stand-in) returned, cast and checked: ``spec`` maps every name to its dtype,
        for (L,), or to (dtype, k), for (k, L)."""
        f = {k: np.ascontiguousarray(got[k], dtype=_dtype(v)) for k, v in spec.items()}
        if any(f[k].shape != _lead(v) + (self.L,) for k, v in spec.items()):
            raise XmhwException(f"{who} stage returned arrays that do not fit {self.L} entries")
        return f


def _dtype(v):
    return v[0] if isinstance(v, tuple) else v


def _lead(v):
    return (v[1],) if isinstance(v, tuple) else ()


def stage_inputs(spec, *arrays):
    """the arguments of a device stage as contiguous arrays of the dtypes of ``spec`` (name -> dtype, in their order)"""
    return [np.ascontiguousarray(a, dtype=t) for a, t in zip(arrays, spec.values())]


@contextmanager
def device_stage(arrays, sizes, too_large):
    """The frame of a device stage: refuses with ``too_large`` where one of ``sizes`` reaches 2**31, then yields (the
    bindings, the DeviceScope of the call, ``arrays`` uploaded, launch); the allocations and the call go under ``with
    launch:``, which turns the bindings' refusals into XmhwExceptions, the read-back behind it."""
    if max(sizes) >= 1 << 31:
        raise XmhwException(f"{too_large}: select fewer objects with ids=")
    h = hip()
    with DeviceScope() as s:
        with as_xmhw_errors(also="Unsupported", hint="select fewer objects with ids="):
            d = [s.upload(a) for a in arrays]
        yield h, s, d, as_xmhw_errors(also="Unsupported", hint="select fewer objects with ids=")
