"""mhw_rank(): counterpart of xmhw.stats.mhw_rank (xmhw/stats.py:446-510, after Hobday's
marineHeatWaves.rank()) on the compact event table of detect() -- which events of a grid cell were the
largest, and how often an event that large comes back.

The reference ranks the dense (events, lat, lon) arrays with ``argsort().argsort()`` along the last axis
(lon, not events), ranks the NaN padding first and fixes the record length at 14245 days.  Here every
ranked column is ranked within each cell by one kernel over the CSR table (csrc/kernels_rank.hip):

    rank_i = 1 + #{j : v_j > v_i} + #{j > i : v_j == v_i}      (1 = largest; of equal values the later
                                                                event ranks first)
    return period = (nYears + 1) / rank

A NaN value gets a NaN rank and return period and does not count for the other events of its cell.
The differences from the reference are deliberate and documented in DESIGN.md.
"""
import numpy as np

from . import calendar as cal
from .detect import EventDataset
from .device import DeviceScope
from .exception import XmhwException
from ._lib import hip

# the reference's rule (stats.py:482-486): every variable whose name holds none of these
_SKIP = ("event", "time", "index")
RANKED = [k for k in EventDataset.columns if not any(x in k for x in _SKIP)]


def record_years(time):
    """Length of the record in years: (time[-1] - time[0] + one step) in days over the year length of the
    record's calendar (365.25, 365, 366 or 360).  One step = time[1] - time[0]; a single-step record is one day."""
    t = np.asarray(time)
    if t.size == 0:
        raise XmhwException("mhw_rank needs a time axis to derive nYears")
    if t.size == 1:
        days = 1.0
    elif t.dtype.kind == "M":
        span = (t[-1] - t[0]) + (t[1] - t[0])
        days = float(span / np.timedelta64(1, "D"))
    elif t.dtype == object and hasattr(t.flat[0], "year"):
        span = (t.flat[-1] - t.flat[0]) + (t.flat[1] - t.flat[0])
        days = span.total_seconds() / 86400.0
    else:
        raise XmhwException("time axis must be datetime64 or cftime-like objects")
    return days / cal.get_calendar(cal.calendar_of(t))


def rank_device(table, offsets, columns, n_years):
    """The device stage on compact arrays: table (n_events, ncol) float64, offsets (C+1,), the table
    columns to rank and nYears.  Returns (rank, return_period), each (n_events, 1 + len(columns)) with
    column 0 left for the caller (the event label)."""
    h = hip()
    table = np.ascontiguousarray(table, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    C = offsets.shape[0] - 1
    n = table.shape[0]
    ncol = len(columns)
    rank = np.empty((n, 1 + ncol))
    rp = np.empty((n, 1 + ncol))
    if C == 0 or n == 0:
        return rank, rp
    with DeviceScope() as s:
        d_tab, d_off = s.upload(table), s.upload(offsets)
        d_rank, d_rp = s.alloc(8 * n * (1 + ncol)), s.alloc(8 * n * (1 + ncol))
        # the kernel writes columns 1.. of every row (ld_out = 1 + ncol), column 0 stays the caller's
        h.event_rank(d_tab.ptr, table.shape[1], d_off.ptr, C, [int(c) for c in columns], float(n_years),
                     d_rank.ptr + 8, d_rp.ptr + 8, 1 + ncol)
        h.stream_sync(0)
        rank = d_rank.to_array((n, 1 + ncol), np.float64)
        rp = d_rp.to_array((n, 1 + ncol), np.float64)
        return rank, rp


def _attrs(name, what):
    if what == "rank":
        return {"long_name": f"rank of {name} within its grid cell (1 = largest)", "units": "1"}
    return {"long_name": f"return period of {name}", "units": "years"}


def mhw_rank(mhw, nYears=None, _compute=None):
    """Rank the events of every grid cell on each event property, from the largest (1) to the smallest,
    and give their return periods.

    ``mhw``: the EventDataset returned by detect().  Ranked are the properties whose name holds none of
    "event", "time", "index" (24 of them, as in the reference).  Within a cell, of equal values the later
    event gets the smaller rank; a NaN value gets a NaN rank.  For cold spells the values are ranked as
    detect() stores them (after its sign flip): rank 1 is the largest stored value, as in the reference.
    ``nYears``: the record length in years for the return period ``(nYears + 1) / rank``; None = the
    length of ``mhw.time`` (plus one step) in days over the year length of its calendar
    (``nYears=14245/365.25`` reproduces the reference's fixed value).  Return periods only make sense for
    a record of many years.

    Returns ``(rank, return_period)``: two EventDataset on the same cells and events as ``mhw``, with the
    columns ``["event", *ranked]``; ``to_dense()`` / ``to_xarray()`` give the reference's layout.
    """
    if not isinstance(mhw, EventDataset):
        raise XmhwException("mhw_rank expects the EventDataset returned by xmhw_amd.detect() "
                            "(a dense xarray Dataset is not ranked)")
    n_years = record_years(mhw.time) if nYears is None else float(nYears)
    if not (np.isfinite(n_years) and n_years > 0):
        raise XmhwException(f"nYears should be a positive number of years, got {nYears}")
    compute = _compute or rank_device
    cols = [mhw.columns.index(k) for k in RANKED]
    rank, rp = compute(mhw.table, mhw.offsets, cols, n_years)
    rank[:, 0] = mhw.table[:, 0]
    rp[:, 0] = mhw.table[:, 0]
    columns = ["event"] + RANKED
    out = []
    for tab, what in ((rank, "rank"), (rp, "return_period")):
        ds = EventDataset(tab, mhw.offsets, mhw.time, mhw.cell_index, mhw.keep, mhw.sdims, mhw.sshape, mhw.coords,
                          dict(mhw.attrs), {k: _attrs(k, what) for k in RANKED}, mhw.coord_attrs, mhw.point)
        ds.columns = columns
        out.append(ds)
    return out[0], out[1]
