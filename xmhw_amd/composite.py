"""mhw_composite(): event-centred composites of a field, per cell -- superposed epoch analysis, the standard tool of the
driver literature (Holbrook et al. 2019; Sen Gupta et al. 2020; the heat-budget composites around onset and decay): what
the SST anomaly, the wind stress, the net heat flux or the mixed-layer depth of a cell look like 30 days before every
heatwave onset of that cell, at the peak, 20 days after the end.  mhw_days_by(), heat_stress() and index_regression()
reduce a cell's series by class of TIME step; this is the reduction by EVENT time.  index_regression() asks which index
drives the anomaly of a cell, the composite asks what happens around the cell's own events.  One pass over the resident
series that requests only the rows of samples some lane needs (csrc/kernels_composite.hip).

The definition.  Inputs: a series ts[T][C]; a base[Dr][C] with row_of_t[T] (one row: a constant per cell); an anchor
bitmap A (one bit per step and cell, the layout of xmhw_event_table_bits); labels class_of_t[T] in [-1, K); before >= 0
and after >= 0 with D = before + after + 1 <= 128; shift in [0, 24].  For every cell c, every anchor step s of c with
k = class_of_t[s] >= 0 and every offset d in [-before, after] with 0 <= s + d < T:
    a = (float64(ts[s + d][c]) - base[row_of_t[s + d]][c]) * 2**-shift        (the scaling is exact)
    a NaN adds nothing; |a| >= 2**7 or infinite adds 1 to n_range; otherwise q = rint(a * 2**16) and, with i = d + before,
    n[k, i, c] += 1 (int32), s[k, i, c] += q (int64), ss[k, i, c] += q**2 (int64).
The class is that of the ANCHOR step, not of the sample: an event belongs to the season or ENSO phase of its onset.
Anchors of class -1 count nowhere, n_range included.  ``shift`` exists because the 2**7 range is an SST range: heat flux
in W m-2 needs shift = 4 or so, and the resolution becomes 2**(shift - 16).  T < 2**17, |q| <= 2**23, q**2 <= 2**46 and at
most T anchors per entry: every sum stays inside 64 bits.  Everything is an integer sum: the result does not depend on
the time blocks, the slabs, the launch geometry or the schedule.

Host side here (validation, the anchor table, class labels, slabs, land, derived fields); device side behind
composite_cells() (a compact host series) and composite_grid() (a stacked grid, masked and compacted on the device).
"""
import numpy as np

from ._lib import hip_composite
from .device import DeviceScope, as_xmhw_errors
from .exception import XmhwException
from .series_stage import (Accumulators, base_series, cell_stage, check_class_ids, check_same_frame, check_steps, check_view,
                           class_labels, class_result_labels, dense_ids, grid_layout, ocean_mask, run_cells, run_grid,
                           stage_attrs, zero_base)
from .trend import p_two_sided

MAX_OFFSETS = 128               # XMHW_COMPOSITE_MAX_OFFSETS (include/xmhw_amd.h)
MAX_CLASSES = 64                # XMHW_COMPOSITE_MAX_CLASSES
MAX_STEPS = 1 << 17             # XMHW_COMPOSITE_MAX_STEPS: T below it
BITS = 16                       # XMHW_COMPOSITE_BITS
RANGE_BITS = 7                  # |a| < 2**7
MAX_SHIFT = 24                  # XMHW_COMPOSITE_MAX_SHIFT
ANCHORS = {"start": "index_start", "peak": "index_peak", "end": "index_end"}
FIELDS = ("n", "s", "ss")
BYTES_PER_ENTRY = 20            # int32 n, int64 s and ss
_ONE = float(1 << BITS)
_RANGE_TEXT = ("samples lie 2**(7 + shift) and more from their base (or are infinite): pass a larger shift (heat flux in "
               "W m-2 needs shift=4 or so)")


# ---- validation (mirrors the refusals of the C entries) ----------------------------------------------

def check_window(before, after, shift):
    """(before, after, shift) as Python ints"""
    for name, v in (("before", before), ("after", after), ("shift", shift)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise XmhwException(f"{name} should be a whole number, got {v!r}")
    before, after, shift = int(before), int(after), int(shift)
    if before < 0 or after < 0:
        raise XmhwException(f"before and after should be >= 0, got {before} and {after}")
    if before + after + 1 > MAX_OFFSETS:
        raise XmhwException(f"mhw_composite handles at most {MAX_OFFSETS} offsets (before + after + 1), got "
                            f"{before + after + 1}")
    if not 0 <= shift <= MAX_SHIFT:
        raise XmhwException(f"shift should be in [0, {MAX_SHIFT}], got {shift}")
    return before, after, shift


def check_result_bytes(K, D, C, max_result_bytes):
    """the (K, D, C) accumulators, 20 bytes an entry, live on the device across the slabs and come back whole"""
    need = BYTES_PER_ENTRY * K * D * C
    if max_result_bytes is not None and need > max_result_bytes:
        raise XmhwException(f"the composite of K = {K} classes x D = {D} offsets x C = {C} cells takes {need} bytes, more "
                            f"than max_result_bytes = {int(max_result_bytes)}: use fewer classes, a shorter window or a "
                            "part of the grid")


# ---- the anchor table --------------------------------------------------------------------------------

def anchor_table(events, anchor="start", select=None):
    """The anchors of an EventDataset as the table that xmhw_event_table_bits rasterises: a dict of n, C, offsets (C + 1,)
    int64, start and end (n,) int32 (start == end == the anchor step; the rows of a cell in time order), cell_index.
    Cells 0 .. C - 2 are the cells of ``events``; cell C - 1 is an empty dummy: the columns of a field that have no table
    cell point at it.  ``anchor``: "start", "peak" or "end" (the columns index_start, index_peak, index_end);
    ``select``: an optional boolean array over the table rows."""
    from .detect import _positions
    if anchor not in ANCHORS:
        raise XmhwException(f"anchor should be one of {tuple(ANCHORS)}, got {anchor!r}")
    view = events.compact_view()
    n, C = view["n"], view["C"]
    step = _positions(events.table[:, events.columns.index(ANCHORS[anchor])], ANCHORS[anchor])
    cell = view["cell_of_row"]
    if select is not None:
        select = np.asarray(select)
        if select.dtype != bool or select.shape != (n,):
            raise XmhwException(f"select should be a boolean array with one entry per event ({n}), got {select.dtype} "
                                f"{select.shape}")
        step, cell = step[select], cell[select]
    # time order within a cell (the table is in that order already; two events of a cell never share an anchor)
    order = np.lexsort((step, cell))
    step, cell = step[order], cell[order]
    offsets = np.zeros(C + 2, dtype=np.int64)
    offsets[1:C + 1] = np.cumsum(np.bincount(cell, minlength=C))
    offsets[C + 1] = offsets[C]
    step = np.ascontiguousarray(step, dtype=np.int32)
    return dict(n=int(step.shape[0]), C=C + 1, offsets=offsets, start=step, end=step, cell_index=view["cell_index"],
                cell_of_row=cell)


def table_cell_of_point(view, N):
    """(N,) int64: the table cell of every grid point, the dummy cell where the table has none"""
    out = np.full(N, view["C"] - 1, dtype=np.int64)
    out[view["cell_index"]] = np.arange(view["C"] - 1, dtype=np.int64)
    return out


# ---- the device stage --------------------------------------------------------------------------------

class _Accumulators(Accumulators):
    """One call's arguments, its anchor table on the device and its accumulators n, s, ss (K, D, C) with the range
    counter; each slab rasterises its own anchor bitmap."""
    range_texts = {"n_range": _RANGE_TEXT}

    def __init__(self, view, cells, classes, K, before, after, shift, max_result_bytes):
        super().__init__()
        self.hc = hip_composite()
        self.view, self.cells = view, np.ascontiguousarray(cells, dtype=np.int64)
        self.args = (classes, K)
        self.before, self.after, self.shift = check_window(before, after, shift)
        self.D = self.before + self.after + 1
        self.max_result_bytes = max_result_bytes

    def begin(self, T, C):
        """T steps, C ocean cells"""
        check_steps(T, "mhw_composite")
        self.classes, self.K = check_class_ids(T, *self.args, MAX_CLASSES, "mhw_composite")
        check_view(self.view, self.cells, T, "events")
        check_result_bytes(self.K, self.D, C, self.max_result_bytes)
        s, v = self._scope, self.view
        self.d_start = s.upload(v["start"] if v["n"] > 0 else np.zeros(1, np.int32))
        self.d_off = s.upload(v["offsets"])
        self.make(C, {k: ((self.K, self.D, C), np.int32 if k == "n" else np.int64) for k in FIELDS})
        with as_xmhw_errors(also="Unsupported"):
            self.hc.composite_init(self.K, self.D, C, *self.ptrs(), C, self.count.ptr)

    def add_slab(self, slab):
        """One slab (series_stage.Slab), columns k0..k0+n-1 of the accumulators: the anchors of its cells are rasterised
        from the table, then the composite ADDS; the base is where the slab carries its climatologies."""
        T, n = slab.T, slab.n
        W = (T + 63) // 64
        ptrs = self.ptrs(slab.k0)
        with DeviceScope() as s:
            d_cell = s.upload(np.ascontiguousarray(slab.take(self.cells), dtype=np.int64))
            d_bits = s.alloc(8 * W * n)
            with as_xmhw_errors(also="Unsupported"):
                self.h.event_table_bits(self.d_start.ptr, self.d_start.ptr, self.d_off.ptr, d_cell.ptr, n, T, d_bits.ptr, n)
                self.hc.composite_accumulate(slab.d_ts.ptr, slab.isz, T, n, slab.ld, slab.se_ptr, slab.ldc, slab.D, slab.rows,
                                             self.shift, d_bits.ptr, n, self.classes, self.K, self.before, self.after, *ptrs,
                                             self.C, self.count.ptr)
            self.h.stream_sync(0)                       # the slab's series and bitmap are freed on the way out


def _bytes_per_cell(T, isz, D):
    return T * isz + T // 8 + 2 * D * 8 + 64


def composite_cells(ts, base, doy, doys, view, cells, classes, K, before, after, shift=0, max_batch_bytes=64 << 30, pad=None,
                    counters=None, max_result_bytes=None):
    """The device stage for a dense (T, C) series: base (Dr, C) with the labels doy (T,) / doys (Dr,) that pair steps and
    base rows as in detect_front.detect_cells, ``view`` an anchor_table(), ``cells`` (C,) the table cell of every column
    (the dummy cell for a column without events), classes (T,) int labels in [-1, K).  Returns n int32, s and ss int64,
    all (K, D, C).  Cells go through the device in batches below max_batch_bytes; the sums are integers, so the batch
    size does not change a single bit.  Raises if a sample is out of range (module docstring); with ``counters`` (a dict)
    it stores ``n_range`` there instead."""
    return run_cells(_Accumulators(view, cells, classes, K, before, after, shift, max_result_bytes), ts, base, base, doy, doys,
                     _bytes_per_cell, max_batch_bytes, pad, counters)


def composite_grid(stacked, anynans, base, doy, doys, view, cells, classes, K, before, after, shift=0, max_batch_bytes=None,
                   clim_stacked=False, pad=None, counters=None, max_result_bytes=None):
    """composite_cells() for an UNCOMPACTED stacked host series (T, N), float or a packed int16 view: the land mask and
    the compaction run on the device slab by slab (series_stage.walk_grid); ``cells`` (N,) holds the table cell of every
    grid point and is compacted by each slab's land mask.  Returns the three arrays over the ocean cells and keep[N]."""
    out, keep = run_grid(_Accumulators(view, cells, classes, K, before, after, shift, max_result_bytes), stacked, anynans,
                         base, base, doy, doys, lambda T, D: 4 * D * 8 + T // 8 + 64, max_batch_bytes, clim_stacked, pad,
                         counters)
    return out + (keep,)


# ---- the result --------------------------------------------------------------------------------------

class CompositeDataset:
    """What mhw_composite() returns, as plain arrays over (klass, offset, *spatial dims).

    klass (K,) the class labels (sorted non-negative labels found), offset (D,) = -before .. after in steps, anchor the
    table column the windows are centred on, shift, n_cells_dropped: the cells of ``events`` that are land in the field.
    Raw integers: n int32, sum_q and sumsq_q int64 (klass, offset, ...): the samples that entered, the sum of their
    q = rint(a * 2**(16 - shift)) and of q**2; n_anchors int32 (klass, ...): the anchors of every cell and class, counted
    on the host (n <= n_anchors: windows leave the record, samples are missing).
    Derived float64, NaN where n < 2:
        mean  sum_q / n * 2**(shift - 16)
        std   the sample standard deviation across the events (ddof = 1), in the units of the field
        t     mean / (std / sqrt(n)): the one-sample t statistic against zero across the events
        p     its two-sided p-value, Student's t with n - 1 degrees of freedom.  Computed on first use.
    The test treats the events of a cell as independent samples; overlapping windows and events a few days apart are
    not, and a significance by resampling is out of scope.
    Land: grid lines without an ocean cell are dropped, as in ClassDaysDataset; the float fields are NaN on the remaining
    land cells, integer fields are 0 there and come with the boolean ``keep`` (...) mask of the ocean cells."""

    def __init__(self, klass, offset, n, sum_q, sumsq_q, n_anchors, keep, sdims, coords, anchor="start", shift=0,
                 n_cells_dropped=0, tdim="time", attrs=None):
        self.klass, self.offset = np.asarray(klass), np.asarray(offset)
        self.n, self.sum_q, self.sumsq_q, self.n_anchors = n, sum_q, sumsq_q, n_anchors
        self.keep, self.sdims, self.coords = keep, tuple(sdims), dict(coords)
        self.anchor, self.shift, self.n_cells_dropped = anchor, int(shift), int(n_cells_dropped)
        self.tdim, self.attrs = tdim, dict(attrs or {})
        self._p = None
        unit = 2.0 ** (self.shift - BITS)
        nf, sq, ssq = n.astype(np.float64), sum_q.astype(np.float64), sumsq_q.astype(np.float64)
        few = n < 2
        with np.errstate(divide="ignore", invalid="ignore"):
            m = sq / nf
            var = np.maximum(ssq - sq * m, 0.0) / (nf - 1.0)
            self.mean = np.where(few, np.nan, m * unit)
            self.std = np.where(few, np.nan, np.sqrt(var) * unit)
            self.t = np.where(few, np.nan, self.mean / (self.std / np.sqrt(nf)))

    @property
    def p(self):
        if self._p is None:
            dof = np.where(self.n < 2, np.nan, self.n.astype(np.float64) - 1.0)
            with np.errstate(invalid="ignore"):
                self._p = p_two_sided(self.t, dof)
        return self._p

    def to_xarray(self):
        import xarray as xr
        cell = ("klass", "offset") + self.sdims
        data = {k: (cell, getattr(self, k)) for k in ("n", "sum_q", "sumsq_q", "mean", "std", "t", "p")}
        data.update(n_anchors=(("klass",) + self.sdims, self.n_anchors), keep=(self.sdims, self.keep))
        return xr.Dataset(data, coords=dict({"klass": self.klass, "offset": self.offset},
                                            **{d: self.coords[d] for d in self.sdims if d in self.coords}),
                          attrs=dict(self.attrs, anchor=self.anchor, shift=self.shift, n_cells_dropped=self.n_cells_dropped))


# ---- the public function -----------------------------------------------------------------------------

def mhw_composite(field, base, events, anchor="start", before=30, after=30, classes="all", select=None, shift=0,
                  tdim="time", maxPadLength=None, tstep=False, anynans=False, max_batch_bytes=None,
                  max_result_bytes=8 << 30, _compute=None):
    """Event-centred composites: per cell, class and offset d in [-before, after], the count, mean and spread of
    ``field - base`` over the steps that lie d steps from an event of that cell.

    ``field`` and ``base`` are taken as index_regression() takes ``temp`` and ``base``: land masking, padding, a constant
    base per cell or a ('doy', ...) climatology such as ``seas`` of threshold(); ``base=None`` is a base of zero.
    ``events``: the EventDataset of a detect() on the same grid and time axis.  ``anchor``: "start", "peak" or "end" --
    the step of every event the offsets count from.  ``select``: an optional boolean array over the rows of
    ``events.table`` (only the events of category 2 and more, only the long ones).  ``classes``: as in mhw_days_by(), at
    most 64; an event belongs to the class of its anchor step.  ``shift``: samples enter as (field - base) * 2**-shift and
    must then lie inside (-2**7, 2**7); the resolution is 2**(shift - 16).  The (klass, offset, cells) accumulators take 20
    bytes an entry: the call raises if that exceeds ``max_result_bytes``.  Cells of ``events`` that are land in ``field``
    are left out and counted in ``n_cells_dropped``.

    Returns a CompositeDataset.  Raises if a sample is out of range.  ``_compute``: a stand-in for composite_cells()
    (host tests)."""
    from .detect import EventDataset
    layout = grid_layout(field, tdim)
    coords, _, dims, point, sdims, sshape, N = layout
    time = np.asarray(coords[tdim])
    T = time.shape[0]
    check_steps(T, "mhw_composite")
    before, after, shift = check_window(before, after, shift)
    D = before + after + 1
    if not isinstance(events, EventDataset):
        raise XmhwException("mhw_composite expects the EventDataset returned by xmhw_amd.detect()")
    check_same_frame("mhw_composite", "field", "events", (point, sdims, sshape), time,
                     (events.point, events.sdims, events.sshape), events.time)
    found, kid, K = dense_ids(class_labels(classes, time), MAX_CLASSES, "mhw_composite", "classes")
    view = anchor_table(events, anchor, select)
    of_point = np.zeros(1, dtype=np.int64) if point else table_cell_of_point(view, N)
    check_view(view, of_point, T, "events")
    if base is None:
        base = zero_base(ocean_mask(field, dims, tdim, point, anynans), point, sdims, sshape, coords)
    base = base_series(base, point, sdims, coords)
    more = (kid, K, before, after, shift)

    def on_cells(host_keep, ts, sec, thc, doy, doys, options, **extra):
        check_result_bytes(K, D, ts.shape[1], max_result_bytes)
        return (_compute or composite_cells)(ts, sec, doy, doys, view, of_point[host_keep()], *more,
                                             max_result_bytes=max_result_bytes, **extra)

    f, arrays, mhw = cell_stage(
        "composite", field, base, base, layout, tdim, on_cells,
        lambda stacked, anynans_, sec, thc, doy, doys, options, **extra:
            composite_grid(stacked, anynans_, sec, doy, doys, view, of_point, *more, max_result_bytes=max_result_bytes,
                           **extra),
        lambda C: [(K, D, C)] * 3, _Accumulators.range_texts, maxPadLength=maxPadLength, tstep=tstep, anynans=anynans,
        _compute=_compute, max_batch_bytes=max_batch_bytes)
    n, s, ss = (f.place(a, 0, np.int32 if k == "n" else np.int64) for k, a in zip(FIELDS, arrays))
    # the anchors of every class and cell of the field, from the table
    cells = of_point[np.asarray(mhw.cell_index, dtype=np.int64)]
    per_table_cell = np.zeros((K, view["C"]), dtype=np.int64)
    k_of_row = kid[view["start"]]
    np.add.at(per_table_cell, (k_of_row[k_of_row >= 0], view["cell_of_row"][k_of_row >= 0]), 1)
    n_anchors = f.place(per_table_cell[:, cells], 0, np.int32)
    field_keep = np.asarray(mhw.keep, dtype=bool).reshape(-1)
    dropped = 0 if point else int((~field_keep[view["cell_index"]]).sum())
    return CompositeDataset(class_result_labels(found), np.arange(-before, after + 1), n, s, ss, n_anchors, f.keep, f.sdims,
                            f.coords, anchor, shift, dropped, tdim, stage_attrs(classes, mhw))
