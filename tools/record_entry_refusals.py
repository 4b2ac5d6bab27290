"""What the bindings of _xmhw_hip answer before their first HIP call: every refusal (exception class and full message) and
every zero-size early return of every entry that takes a device pointer, for float32 and float64 where the entry is typed.
Pure host code: device pointers are plain integers -- 0 where a NULL is the point, otherwise a value nothing dereferences.

    python tools/record_entry_refusals.py                  writes tests/golden/entry_refusals.json
    python tools/record_entry_refusals.py --replay OUT     (the child) runs the table into OUT

tests/test_host_entry_refusals.py replays the table and compares.  The table runs in a child process that sees no device
(HIP_VISIBLE_DEVICES=-1) and checks that first: a case that slips past its check meets a runtime without a device, never
a kernel.  Such a case ends in HipError, which the recorder refuses to write."""
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "entry_refusals.json")

P = 0x1000                  # a "device pointer": never dereferenced by a case of this table
BIG = 1 << 31               # the first count the 2^31 limits refuse
T, C, D, K = 8, 3, 4, 2
ROWS = (np.arange(T) % D).astype(np.int32)
CLASSES = (np.arange(T) % K).astype(np.int32)
LAGS = np.array([0, 1], np.int32)

# bindings that take no device pointer (handles of plans, streams and events, host memory, switches, introspection)
NO_DEVICE_POINTER = frozenset("""version arch device_count set_device get_device device_info malloc stream_create stream_sync
    event_create event_destroy event_record stream_wait_event event_elapsed_ms event_sync plan_create host_alloc host_view
    clim_host debug_stats_available sorted_device_ok release_cached_tables set_exceed_kernel set_region_wave_sum
    set_track_intensity_combine set_class_days_block set_cooccur_block set_displacement_block""".split())
# the sharded path: a communicator cannot exist without RCCL and devices
COMM = frozenset("""comm_unique_id comm_create comm_destroy comm_allgather_i64 comm_allgather_bytes gather_blocks""".split())


def module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("xmhw_amd._xmhw_hip")


class Entry:
    """One binding: a call that passes every check (never made), and the changes to it that make the cases."""

    def __init__(self, name, base, cases, nulls=(), typed=False, positional=False, itemsizes=(4, 8), bad_itemsize=3):
        self.name, self.base, self.positional = name, base, positional
        self.cases = [(label, dict(change)) for label, change in cases]
        self.cases += [(f"NULL {p}", {p: 0}) for p in nulls]
        self.sizes = itemsizes if typed else (None,)
        if typed:
            self.cases.append(("bad itemsize", {"itemsize": bad_itemsize}))

    def calls(self):
        for size in self.sizes:
            for label, change in self.cases:
                kw = dict(self.base)
                if size is not None:
                    kw["itemsize"] = size
                kw.update(change)
                yield f"{self.name}{'' if size is None else f'[{size}]'}: {label}", kw


def _stage(**extra):
    """the arguments most detect-side entries share"""
    kw = dict(ts=P, itemsize=4, T=T, C=C, ld=C)
    kw.update(extra)
    return kw


def table(h):
    plan = h.plan_create(np.tile(np.arange(1, 40), 3).astype(np.int32), 1)      # 3 tracks: no sorted-list kernel
    md = [("minDuration 0", dict(min_duration=0)), ("maxGap -1", dict(max_gap=-1))]
    E = []

    def add(*a, **k):
        E.append(Entry(*a, **k))


    # ---- memory
    add("free", dict(p=0), [("NULL returns", {})], positional=True)
    add("host_free", dict(p=0), [("NULL returns", {})], positional=True)
    add("memcpy_h2d", dict(dst=P, src=np.zeros(0)), [("no bytes", {})])
    add("memcpy_d2h", dict(dst=np.zeros(0), src=P), [("no bytes", {})])
    add("memcpy_h2d_async", dict(dst=P, src=P, bytes=0, stream=0), [("no bytes", {})], positional=True)
    add("memset", dict(dst=P, value=0, nbytes=0), [("no bytes", {})])
    a2 = np.zeros((4, 6))
    add("memcpy2d_h2d", dict(dst=P, src=a2, col0=1, ncols=2),
        [("1-D source", dict(src=np.zeros(4))), ("strided rows", dict(src=a2[:, ::2])), ("col0 < 0", dict(col0=-1)),
         ("columns past the end", dict(col0=5)), ("both: 1-D and columns", dict(src=np.zeros(4), col0=-1)),
         ("no columns", dict(ncols=0)), ("NULL dst", dict(dst=0))])
    for name in ("memcpy2d_d2h", "memcpy2d_d2h_async"):
        add(name, dict(dst=a2, col0=1, ncols=2, src=P),
            [("1-D destination", dict(dst=np.zeros(4))), ("not contiguous", dict(dst=a2[:, :4])),
             ("ncols < 0", dict(ncols=-1)),
             ("columns past the end", dict(col0=5)), ("no columns", dict(ncols=0)), ("NULL src", dict(src=0))])
    add("read_rows", dict(fd=0, file_offset=0, row_pitch=8, row_bytes=8, rows=2, dst=P),
        [("bad fd", dict(fd=-1)), ("pitch < row", dict(row_pitch=4)), ("no rows", dict(rows=0)), ("NULL dst", dict(dst=0)),
         ("both: bad fd and NULL", dict(fd=-1, dst=0))])
    # ---- plans (their handle passes through the same pointer argument)
    for name, rest in (("plan_destroy", ()), ("plan_info", ()), ("plan_doys", ()), ("plan_set_kernel", (0,)),
                       ("plan_set_narrowing", (1,)), ("plan_narrowed", ()), ("plan_set_chunks", (0,)), ("plan_table", (6,)),
                       ("plan_set_timing", (1,)), ("plan_kernel_ms", (0,)), ("plan_sorted_info", (1,)),
                       ("plan_sorted_table", (1,)), ("plan_debug_stats", (0, False)), ("plan_chunks_in_use", (1,)),
                       ("plan_set_layout", (8,)), ("plan_layout_in_use", ()), ("plan_f64_mode", ()),
                       ("plan_route", (4, 0.9, 1))):
        add(name, dict(enumerate((0,) + rest)), [("NULL plan", {})], positional=True)
    # ---- threshold
    add("clim_raw", dict(plan=plan, ts=P, itemsize=4, C=C, ld=C, q=0.9, negate=0, thresh=P, seas=P, ldo=C),
        [("NULL plan", dict(plan=0)), ("C < 0", dict(C=-1)), ("ld < C", dict(ld=2)), ("ldo < C", dict(ldo=2)),
         ("q > 1", dict(q=1.5)), ("q NaN", dict(q=float("nan"))), ("both: bad ld and q", dict(ld=2, q=2.0)),
         ("both: bad itemsize and NULL plan", dict(itemsize=3, plan=0)), ("C == 0", dict(C=0)),
         ("both: C == 0 and NULL", dict(C=0, ts=0))], nulls=("ts", "thresh", "seas"), typed=True)
    add("clim_raw_i16", dict(plan=plan, codes=P, C=C, ld=C, big_endian=0, has_scale=1, scale_factor=0.01, add_offset=0.0,
                             has_fill=1, fill_code=-32768, decoded_itemsize=4, q=0.9, negate=0, thresh=P, seas=P, ldo=C),
        [("NULL plan", dict(plan=0)), ("ld < C", dict(ld=2)), ("q < 0", dict(q=-0.1)),
         ("decoded_itemsize 2", dict(decoded_itemsize=2)),
         ("scale 0", dict(scale_factor=0.0)), ("offset NaN", dict(add_offset=float("nan"))), ("C == 0", dict(C=0)),
         ("both: bad q and decoded_itemsize", dict(q=2.0, decoded_itemsize=2)), ("no sorted-list kernel for the plan", {})],
        nulls=("codes", "thresh", "seas"))
    add("clim_finish", dict(plan=plan, thresh_in=P, seas_in=P, C=C, ldo=C, feb29_fix=1, smooth=1, width=31, thresh_out=2 * P,
                            seas_out=2 * P),
        [("NULL plan", dict(plan=0)), ("even window", dict(width=30)), ("ldo < C", dict(ldo=2)), ("C == 0", dict(C=0)),
         ("both: even window and bad ldo", dict(width=30, ldo=2)), ("thresh aliases", dict(thresh_out=P)),
         ("seas aliases", dict(seas_out=P))], nulls=("thresh_in", "seas_in", "thresh_out", "seas_out"))
    add("land_mask", dict(ts=P, itemsize=4, T=T, C=C, ld=C, anynans=0, keep=P),
        [("T == 0", dict(T=0)), ("C < 0", dict(C=-1)), ("ld < C", dict(ld=2))], typed=True)
    add("land_mask_i16", dict(codes=P, T=T, C=C, ld=C, big_endian=0, has_fill=1, fill_code=-1, anynans=0, keep=P),
        [("T == 0", dict(T=0)), ("ld < C", dict(ld=2)), ("fill_code not int16", dict(fill_code=40000)),
         ("C == 0", dict(C=0)),
         ("both: bad fill and C == 0", dict(fill_code=40000, C=0))], nulls=("codes", "keep"))
    add("gather_cells", {"in": P, "itemsize": 4, "rows": 2, "ld_in": C, "index": P, "n": C, "out": P, "ld_out": C},
        [("rows < 0", dict(rows=-1)), ("n < 0", dict(n=-1)), ("ld_out < n", dict(ld_out=2))], typed=True,
        itemsizes=(2, 4, 8))
    add("scatter_cells", {"in": P, "rows": 2, "ld_in": C, "index": P, "n": C, "out": P, "ld_out": C},
        [("rows < 0", dict(rows=-1)), ("ld_in < n", dict(ld_in=2))])
    add("synth_sst", dict(ts=P, itemsize=4, T=T, C=C, ld=C, cell0=0, seed=1),
        [("T == 0", dict(T=0)), ("ld < C", dict(ld=2))],
        typed=True)
    add("synth_sst_ex", dict(ts=P, T=T, C=C, ld=C, cell0=0, seed=1),
        [("NULL ts", dict(ts=0)), ("T < 0", dict(T=-1)), ("rho 1", dict(rho=1.0)), ("ice_frac 2", dict(ice_frac=2.0)),
         ("both: NULL and rho", dict(ts=0, rho=1.0))])
    # ---- ingest
    add("decode", dict(raw=P, raw_itemsize=2, big_endian=0, rows=2, cols=C, ld_raw=C, out=P, out_itemsize=4, ld_out=C,
                       has_scale=True, scale=0.01, offset=0.0, has_fill=False, fill=0.0),
        [("rows < 0", dict(rows=-1)), ("ld_raw < cols", dict(ld_raw=2)), ("no rows", dict(rows=0)),
         ("no cols", dict(cols=0))],
        nulls=("raw", "out"))
    add("encode_i16",
        {"in": P, "rows": 2, "cols": C, "ld_in": C, "out": P, "ld_out": C, "scale": 0.01, "offset": 0.0, "fill": -1},
        [("ld_out < cols", dict(ld_out=2)), ("scale 0", dict(scale=0.0)), ("fill not int16", dict(fill=40000)),
         ("no rows", dict(rows=0)), ("both: bad fill and no rows", dict(fill=40000, rows=0))], nulls=("in", "out"))
    add("pad_gaps", dict(ts=P, itemsize=4, T=T, C=C, ld=C, x=P, max_gap=2.0),
        [("ld < C", dict(ld=2)), ("itemsize 2", dict(itemsize=2)), ("max_gap NaN", dict(max_gap=float("nan"))),
         ("T == 0", dict(T=0)), ("both: bad ld and itemsize", dict(ld=2, itemsize=2))], nulls=("ts", "x"))
    # ---- detect
    short = ROWS[:-1]
    add("detect_events", _stage(thresh=P, ldt=C, row_of_t=ROWS, min_duration=5, join_gaps=1, max_gap=2, negate=0, events=P,
                                start=P, end=P, bthresh=P, ldo=C, nevents=P),
        [("short row_of_t", dict(row_of_t=short)),
         ("both: short row_of_t and bad itemsize", dict(row_of_t=short, itemsize=3)),
         ("ldt < C", dict(ldt=2)), ("ldo < C", dict(ldo=2)), ("C == 0", dict(C=0)),
         ("both: bad ld and minDuration", dict(ld=2, min_duration=0)), ("both: C == 0 and NULL", dict(C=0, ts=0))] + md,
        nulls=("ts", "thresh", "events", "start", "end"), typed=True)
    add("count_events", dict(start=P, T=T, C=C, ldo=C, nevents=P), [("T == 0", dict(T=0)), ("ldo < C", dict(ldo=2)),
                                                                    ("C == 0", dict(C=0))], nulls=("start", "nevents"))
    add("event_stats", _stage(seas=P, thresh=P, ldc=C, row_of_t=ROWS, negate=0, events=P, ldo=C, offsets=P, table=P),
        [("short row_of_t", dict(row_of_t=short)),
         ("both: short row_of_t and bad itemsize", dict(row_of_t=short, itemsize=3)),
         ("ldc < C", dict(ldc=2)), ("C < 0", dict(C=-1)), ("C == 0", dict(C=0)),
         ("both: C == 0 and NULL", dict(C=0, seas=0))],
        nulls=("ts", "seas", "thresh", "events", "offsets"), typed=True)
    add("exceed_bits", _stage(thresh=P, ldt=C, D=D, row_of_t=ROWS, negate=0, bits=P, ldb=C),
        [("short row_of_t", dict(row_of_t=short)),
         ("both: short row_of_t and bad itemsize", dict(row_of_t=short, itemsize=3)),
         ("D == 0", dict(D=0)), ("ldb < C", dict(ldb=2)), ("C == 0", dict(C=0)), ("row >= D", dict(D=3)),
         ("row < 0", dict(row_of_t=ROWS - 1)), ("both: C == 0 and row >= D", dict(C=0, D=3)),
         ("both: NULL and row >= D", dict(bits=0, D=3))], nulls=("ts", "thresh", "bits"), typed=True)
    add("events_from_bits",
        dict(bits=P, T=T, C=C, ldb=C, min_duration=5, join_gaps=1, max_gap=2, offsets=P, nevents=P, table=P),
        [("T == 0", dict(T=0)), ("ldb < C", dict(ldb=2)), ("C == 0", dict(C=0)),
         ("neither offsets nor nevents", dict(offsets=0, nevents=0)),
         ("offsets without table", dict(table=0)), ("both: NULL and minDuration", dict(bits=0, min_duration=0))] + md,
        nulls=("bits",))
    add("event_stats_sparse", _stage(seas=P, thresh=P, ldc=C, row_of_t=ROWS, negate=0, n_events=5, table=P),
        [("short row_of_t", dict(row_of_t=short)),
         ("both: short row_of_t and bad itemsize", dict(row_of_t=short, itemsize=3)),
         ("ld < C", dict(ld=2)), ("n_events < 0", dict(n_events=-1)), ("n_events == 0", dict(n_events=0)),
         ("both: n_events == 0 and NULL", dict(n_events=0, table=0))], nulls=("ts", "seas", "thresh", "table"), typed=True)
    add("event_intermediate", _stage(seas=P, thresh=P, ldc=C, row_of_t=ROWS, negate=0, events=P, ldo=C, out=P, ldv=C, dur=P),
        [("short row_of_t", dict(row_of_t=short)),
         ("both: short row_of_t and bad itemsize", dict(row_of_t=short, itemsize=3)),
         ("ldv < C", dict(ldv=2)), ("T == 0", dict(T=0)), ("C == 0", dict(C=0)),
         ("both: C == 0 and NULL", dict(C=0, out=0))],
        nulls=("ts", "seas", "thresh", "events", "out", "dur"), typed=True)
    # ---- block statistics, ranks, trends, fits
    add("block_events", dict(table=P, offsets=P, C=C, bin_of_t=P, T=T, nbins=2, mtime_col=0, out=P, ldo=C),
        [("nbins == 0", dict(nbins=0)), ("ldo < C", dict(ldo=2)), ("mtime_col -1", dict(mtime_col=-1)),
         ("mtime_col past the row", dict(mtime_col=h.EVENT_COLUMNS)), ("C == 0", dict(C=0)),
         ("both: bad mtime_col and C == 0", dict(mtime_col=-1, C=0))], nulls=("table", "offsets", "bin_of_t", "out"))
    add("block_time", _stage(cats=P, ldcat=C, bin_of_t=P, nbins=2, out=P, ldo=C),
        [("T == 0", dict(T=0)), ("ldcat < C", dict(ldcat=2)), ("no cats: ldcat free", dict(cats=0, ldcat=0, C=0)),
         ("ldo < C", dict(ldo=2)), ("C == 0", dict(C=0))], nulls=("ts", "bin_of_t", "out"), typed=True)
    add("event_rank",
        dict(table=P, ld_table=h.EVENT_COLUMNS, offsets=P, C=C, columns=[3, 4], n_years=30.0, rank=P, rp=P, ld_out=2),
        [("C < 0", dict(C=-1)), ("ld_table 0", dict(ld_table=0)), ("no columns", dict(columns=[])),
         ("32 columns", dict(columns=list(range(31)) + [0], ld_out=32)),
         ("column >= ld_table", dict(columns=[3, h.EVENT_COLUMNS])),
         ("column < 0", dict(columns=[-1])), ("ld_out < ncols", dict(ld_out=1)), ("n_years 0", dict(n_years=0.0)),
         ("n_years inf", dict(n_years=float("inf"))), ("both: bad column and ld_out", dict(columns=[3, 99], ld_out=1)),
         ("C == 0", dict(C=0)), ("both: bad n_years and C == 0", dict(n_years=0.0, C=0))],
        nulls=("table", "offsets", "rank", "rp"))
    trend = dict(y=P, nstat=2, nb=5, C=C, ld=C, x=P, out=P, ldo=C)
    tcases = [("nb < 0", dict(nb=-1)), ("ld < C", dict(ld=2)), ("ldo < C", dict(ldo=2)), ("nstat == 0", dict(nstat=0)),
              ("C == 0", dict(C=0)), ("both: bad ld and ldo", dict(ld=2, ldo=2)), ("NULL out", dict(out=0)),
              ("NULL y", dict(y=0)),
              ("NULL x", dict(x=0)), ("both: NULL out and y", dict(out=0, y=0)),
              ("nstat * C past one launch", dict(nstat=100, C=BIG, ld=BIG, ldo=BIG))]
    add("block_trend_ols", dict(trend, tcrit=P),
        tcases + [("NULL tcrit", dict(tcrit=0)), ("both: NULL tcrit and C == 0", dict(tcrit=0, C=0))])
    add("block_trend_theil_sen", trend,
        tcases + [("nb above the cap", dict(nb=129)), ("both: nb cap and C == 0", dict(nb=129, C=0))])
    fit = _stage(basis=P, P=2, coef=P, ldc=C)
    fcases = [("T < 0", dict(T=-1)), ("P == 0", dict(P=0)), ("P above the cap", dict(P=h.FIT_MAX_TERMS + 1)),
              ("ld < C", dict(ld=2)),
              ("ldc < C", dict(ldc=2)), ("both: bad P and ld", dict(P=0, ld=2)), ("C == 0", dict(C=0)),
              ("T == 0", dict(T=0)),
              ("both: T == 0 and NULL", dict(T=0, ts=0)), ("C past one launch", dict(C=1 << 38, ld=1 << 38, ldc=1 << 38))]
    add("series_fit", dict(fit, weight=P, min_valid=2, nvalid=P), fcases, nulls=("ts", "basis", "coef"), typed=True)
    add("series_remove", dict(fit, R=1),
        fcases + [("R == 0", dict(R=0)), ("R > P", dict(R=3)), ("both: R == 0 and C == 0", dict(R=0, C=0)),
                  ("T past one launch", dict(T=1 << 23))], nulls=("ts", "basis", "coef"),
        typed=True)
    add("offsets_from_counts", dict(counts=P, n=C, offsets=P),
        [("n < 0", dict(n=-1)), ("both: n < 0 and NULL", dict(n=-1, offsets=0))],
        nulls=("counts", "offsets"))
    # ---- coverage, regions
    add("coverage_accumulate",
        _stage(seas=P, thresh=P, ldc=C, row_of_t=ROWS, negate=0, bits=P, ldb=C, min_duration=5, join_gaps=1,
               max_gap=2, wq=P, region=P, R=2, cells=P, area_q=P),
        [("short row_of_t", dict(row_of_t=short)),
         ("both: short row_of_t and bad itemsize", dict(row_of_t=short, itemsize=3)),
         ("ldb < C", dict(ldb=2)), ("R == 0", dict(R=0)), ("R above the cap", dict(R=h.COVERAGE_MAX_REGIONS + 1)),
         ("both: bad ld and R", dict(ld=2, R=0)),
         ("both: minDuration and R cap", dict(min_duration=0, R=h.COVERAGE_MAX_REGIONS + 1)),
         ("C == 0", dict(C=0)), ("both: R cap and C == 0", dict(R=h.COVERAGE_MAX_REGIONS + 1, C=0))] + md,
        nulls=("ts", "seas", "thresh", "bits", "wq", "region", "cells", "area_q"), typed=True)
    add("region_accumulate", _stage(x0=0.0, wi=P, region=P, R=2, acc=P, n_range=P),
        [("T < 0", dict(T=-1)), ("ld < C", dict(ld=2)), ("T 2^31", dict(T=BIG)), ("R == 0", dict(R=0)),
         ("R above the cap", dict(R=h.REGION_MAX_REGIONS + 1)), ("x0 NaN", dict(x0=float("nan"))),
         ("x0 inf", dict(x0=float("inf"))),
         ("both: R cap and x0", dict(R=h.REGION_MAX_REGIONS + 1, x0=float("nan"))), ("C == 0", dict(C=0)),
         ("T == 0", dict(T=0)),
         ("both: x0 and T == 0", dict(x0=float("nan"), T=0))], nulls=("ts", "wi", "region", "acc", "n_range"), typed=True)
    # ---- objects
    add("event_objects", dict(start=P, end=P, n=5, offsets=P, C=C, nbr=P, K=4, gap=0, cell_of_row=P, root=P),
        [("n < 0", dict(n=-1)), ("K == 0", dict(K=0)), ("gap < 0", dict(gap=-1)), ("n 2^31", dict(n=BIG)),
         ("C 2^31", dict(C=BIG)),
         ("both: K and 2^31", dict(K=0, n=BIG)), ("n == 0", dict(n=0)), ("rows without cells", dict(C=0)),
         ("both: n == 0 and C == 0", dict(n=0, C=0))], nulls=("start", "end", "offsets", "nbr", "cell_of_row", "root"))
    add("object_reduce",
        dict(start=P, end=P, imax=P, n=5, cell_of_row=P, offsets=P, wq=P, slot=P, n_slots=2, n_events=P, n_cells=P,
             time_start=P, time_end=P, cell_days=P, area_days_q=P, intensity_max=P, peak_row=P),
        [("n < 0", dict(n=-1)), ("n_slots < 0", dict(n_slots=-1)), ("n 2^31", dict(n=BIG)),
         ("n_slots 2^31", dict(n_slots=BIG)),
         ("n_slots == 0", dict(n_slots=0)), ("both: n_slots == 0 and NULL", dict(n_slots=0, n_events=0)),
         ("both: NULL output and input", dict(peak_row=0, start=0))],
        nulls=("n_events", "n_cells", "time_start", "time_end", "cell_days", "area_days_q", "intensity_max", "peak_row",
               "start",
               "end", "imax", "cell_of_row", "offsets", "wq", "slot"))
    rows_in = ("start", "end", "slot", "cell_of_row")
    add("object_tracks",
        dict(start=P, end=P, n=5, slot=P, cell_of_row=P, C=C, vec=P, ldv=C, time_start=P, offsets=P, n_slots=2, L=6,
             n_cells=P, sums=P, ld=7, n_bad=P),
        [("L < 0", dict(L=-1)), ("n 2^31", dict(n=BIG)), ("n_slots 2^31", dict(n_slots=BIG)),
         ("L + 1 2^31", dict(L=BIG - 1, ld=BIG)),
         ("ld < L + 1", dict(ld=6)), ("ldv < C", dict(ldv=2)), ("both: 2^31 and bad ld", dict(n=BIG, ld=6)),
         ("both: bad ld and NULL", dict(ld=6, sums=0))],
        nulls=("n_cells", "sums", "n_bad") + rows_in + ("vec", "time_start", "offsets"))
    vox = dict(start=P, end=P, slot=P, cell_of_row=P, n=5, row_offsets=P, C=C, nbr=P, K=4)
    tail = dict(time_start=P, offsets=P, n_slots=2, L=6)
    ocases = [("V < 0", dict(V=-1)), ("K == 0", dict(K=0)), ("n 2^31", dict(n=BIG)), ("C 2^31", dict(C=BIG)),
              ("n_slots 2^31", dict(n_slots=BIG)),
              ("L 2^31", dict(L=BIG)), ("V 2^31", dict(V=BIG)), ("both: K and 2^31", dict(K=0, V=BIG)),
              ("both: 2^31 and NULL", dict(L=BIG, n_bad=0))]
    add("object_parts", dict(vox, wq=P, vox_off=P, V=9, **tail, n_parts=P, cells_largest=P, area_largest_q=P, n_bad=P),
        ocases,
        nulls=("n_bad", "n_parts", "cells_largest", "area_largest_q") + rows_in + ("row_offsets", "nbr", "wq", "vox_off",
                                                                                   "time_start", "offsets"))
    add("object_genealogy",
        dict(vox, vox_off=P, V=9, **tail, counts=P, edges=P, edge_capacity=4, n_edges=P, n_bad=P, overflow=P),
        ocases + [("edge_capacity < 0", dict(edge_capacity=-1)), ("edge_capacity 2^31", dict(edge_capacity=BIG))],
        nulls=("n_bad", "overflow", "n_edges", "counts", "edges") + rows_in + ("row_offsets", "nbr", "vox_off", "time_start",
                                                                               "offsets"))
    add("object_shape",
        dict(start=P, end=P, slot=P, cell_of_row=P, n=5, row_offsets=P, C=C, faces=P, K=4, lq=P, **tail, edges=P,
             perimeter_q=P, cells_edge=P, n_bad=P),
        [("n < 0", dict(n=-1)), ("K 8", dict(K=8)), ("both: bad n and K", dict(n=-1, K=8)), ("n 2^31", dict(n=BIG)),
         ("C 2^31", dict(C=BIG)),
         ("L 2^31", dict(L=BIG)), ("both: K and 2^31", dict(K=8, C=BIG))],
        nulls=("n_bad", "edges", "perimeter_q", "cells_edge") + rows_in + ("row_offsets", "faces", "lq", "time_start",
                                                                           "offsets"))
    # ---- track intensity
    ti_out = dict(n_valid=P, wsum_i=P, isum_q=P, intensity_max=P, cat_cells=P, ldcat=6, n_range=P, n_bad=P)
    add("track_intensity_init", dict(L=6, **ti_out),
        [("L < 0", dict(L=-1)), ("ldcat < L", dict(ldcat=5)), ("L 2^31", dict(L=BIG, ldcat=BIG)),
         ("both: 2^31 and NULL", dict(L=BIG, ldcat=BIG, n_bad=0))],
        nulls=("n_range", "n_bad", "n_valid", "wsum_i", "isum_q", "intensity_max", "cat_cells"))
    add("track_intensity_accumulate",
        dict(ts=P, itemsize=4, T=T, n=C, ld=C, seas=P, thresh=P, ldc=C, D=D, row_of_t=ROWS, negate=0, start=P, end=P, slot=P,
             n_rows=5,
             row_offsets=P, wi=P, time_start=P, offsets=P, n_slots=2, L=6, **ti_out),
        [("short row_of_t", dict(row_of_t=short)),
         ("both: short row_of_t and bad itemsize", dict(row_of_t=short, itemsize=3)),
         ("ld < n", dict(ld=2)), ("D == 0", dict(D=0)), ("n_rows < 0", dict(n_rows=-1)), ("ldcat < L", dict(ldcat=5)),
         ("both: bad ld and ldcat", dict(ld=2, ldcat=5)), ("n 2^31", dict(n=BIG, ld=BIG, ldc=BIG)),
         ("n_rows 2^31", dict(n_rows=BIG)),
         ("n_slots 2^31", dict(n_slots=BIG)), ("L 2^31", dict(L=BIG, ldcat=BIG)), ("n == 0", dict(n=0)),
         ("n_rows == 0", dict(n_rows=0)),
         ("n_slots == 0", dict(n_slots=0)), ("L == 0", dict(L=0)), ("both: L == 0 and row >= D", dict(L=0, D=3)),
         ("both: NULL input and output", dict(ts=0, n_bad=0)), ("row >= D", dict(D=3)), ("row < 0", dict(row_of_t=ROWS - 1)),
         ("both: NULL output and row >= D", dict(n_bad=0, D=3))],
        nulls=("ts", "seas", "thresh", "start", "end", "slot", "row_offsets", "wi", "time_start", "offsets", "n_valid",
               "wsum_i",
               "isum_q", "intensity_max", "cat_cells", "n_range", "n_bad"), typed=True)
    add("track_intensity_finish", dict(L=6, intensity_max=P),
        [("L < 0", dict(L=-1)), ("L 2^31", dict(L=BIG)), ("L == 0", dict(L=0))],
        nulls=("intensity_max",))
    # ---- days by class
    kmax = h.CLASS_DAYS_MAX_CLASSES
    cd_out = dict(days=P, isum_q=P, intensity_max=P, ldo=C, n_range=P)
    add("class_days_init", dict(K=K, C=C, **cd_out),
        [("K == 0", dict(K=0)), ("K above the cap", dict(K=kmax + 1)), ("C 2^31", dict(C=BIG, ldo=BIG)),
         ("C < 0", dict(C=-1)),
         ("ldo < C", dict(ldo=2)), ("both: K and ldo", dict(K=0, ldo=2)),
         ("both: 2^31 and NULL", dict(C=BIG, ldo=BIG, n_range=0))],
        nulls=("n_range", "days", "isum_q", "intensity_max"))
    far = CLASSES + 1
    add("class_days_accumulate",
        _stage(seas=P, thresh=P, ldc=C, row_of_t=ROWS, negate=0, bits=P, ldb=C, min_duration=5, join_gaps=1,
               max_gap=2, class_of_t=CLASSES, K=K, **cd_out),
        [("short row_of_t", dict(row_of_t=short)), ("short class_of_t", dict(class_of_t=CLASSES[:-1])),
         ("both: short row_of_t and class_of_t", dict(row_of_t=short, class_of_t=CLASSES[:-1])),
         ("all: bad itemsize, short row_of_t, class >= K", dict(itemsize=3, row_of_t=short, class_of_t=far)),
         ("both: bad itemsize and class >= K", dict(itemsize=3, class_of_t=far)),
         ("K == 0", dict(K=0)), ("K above the cap", dict(K=kmax + 1)),
         ("C 2^31", dict(C=BIG, ld=BIG, ldc=BIG, ldb=BIG, ldo=BIG)),
         ("both: K and bad ld", dict(K=0, ld=2)), ("ldo < C", dict(ldo=2)), ("class >= K", dict(class_of_t=far)),
         ("class < -1", dict(class_of_t=CLASSES - 2)), ("class -1 passes, C == 0", dict(class_of_t=CLASSES - 1, C=0)),
         ("both: minDuration and class >= K", dict(min_duration=0, class_of_t=far)), ("C == 0", dict(C=0)),
         ("both: class >= K and C == 0", dict(class_of_t=far, C=0)),
         ("both: class >= K and NULL", dict(class_of_t=far, ts=0))] + md,
        nulls=("ts", "seas", "thresh", "bits", "days", "isum_q", "intensity_max", "n_range"), typed=True)
    add("class_days_finish", dict(K=K, C=C, intensity_max=P, ldo=C),
        [("K == 0", dict(K=0)), ("C 2^31", dict(C=BIG, ldo=BIG)), ("ldo < C", dict(ldo=2)), ("C == 0", dict(C=0)),
         ("both: K and C == 0", dict(K=0, C=0))], nulls=("intensity_max",))
    # ---- co-occurrence
    add("event_table_bits", dict(start=P, end=P, offsets=P, cell=P, C=C, T=T, bits=P, ldb=C),
        [("T 2^31", dict(T=BIG)), ("C 2^31", dict(C=BIG, ldb=BIG)), ("T < 0", dict(T=-1)), ("ldb < C", dict(ldb=2)),
         ("C == 0", dict(C=0)),
         ("T == 0", dict(T=0)), ("both: 2^31 and bad ldb", dict(T=BIG, ldb=2))], nulls=("offsets", "cell", "bits"))
    add("cooccur_init", dict(K=K, L=2, C=C, counts=P, ldo=C),
        [("K == 0", dict(K=0)), ("K above the cap", dict(K=h.COOCCUR_MAX_CLASSES + 1)), ("L == 0", dict(L=0)),
         ("L above the cap", dict(L=h.COOCCUR_MAX_LAGS + 1)), ("C 2^31", dict(C=BIG, ldo=BIG)), ("C < 0", dict(C=-1)),
         ("ldo < C", dict(ldo=2)),
         ("both: K and L", dict(K=0, L=0)), ("both: L and C < 0", dict(L=0, C=-1)), ("C == 0", dict(C=0))],
        nulls=("counts",))
    add("cooccur_accumulate",
        dict(a_bits=P, lda=C, b_bits=P, ldb=C, T=T, C=C, class_of_t=CLASSES, K=K, lags=LAGS, counts=P, ldo=C),
        [("short class_of_t", dict(class_of_t=CLASSES[:-1])),
         ("both: short class_of_t and K", dict(class_of_t=CLASSES[:-1], K=0)),
         ("K == 0", dict(K=0)), ("no lags", dict(lags=LAGS[:0])),
         ("lags above the cap", dict(lags=np.zeros(h.COOCCUR_MAX_LAGS + 1, np.int32))),
         ("C 2^31", dict(C=BIG, lda=BIG, ldb=BIG, ldo=BIG)), ("lda < C", dict(lda=2)), ("ldo < C", dict(ldo=2)),
         ("class >= K", dict(class_of_t=far)), ("class < -1", dict(class_of_t=CLASSES - 2)),
         ("both: bad lda and class >= K", dict(lda=2, class_of_t=far)),
         ("C == 0", dict(C=0)), ("T == 0", dict(T=0, class_of_t=CLASSES[:0])),
         ("both: class >= K and C == 0", dict(class_of_t=far, C=0)),
         ("both: class >= K and NULL", dict(class_of_t=far, counts=0))], nulls=("a_bits", "b_bits", "counts"))
    # ---- displacement
    dmax = h.DISPLACEMENT_MAX_CLASSES
    d_out = dict(n_days=P, n_found=P, sum_m=P, sum_north_m=P, sum_east_m=P, max_m=P, ldo=C, n_visited=P)
    add("displacement_init", dict(K=K, C=C, **d_out),
        [("K == 0", dict(K=0)), ("K above the cap", dict(K=dmax + 1)), ("C 2^31", dict(C=BIG, ldo=BIG)),
         ("C < 0", dict(C=-1)), ("ldo < C", dict(ldo=2)),
         ("both: K and ldo", dict(K=0, ldo=2))],
        nulls=("n_visited", "n_days", "n_found", "sum_m", "sum_north_m", "sum_east_m", "max_m"))
    axis = h.DISPLACEMENT_MAX_AXIS
    add("displacement_accumulate",
        dict(ts=P, itemsize=4, ld=6, t0=0, nt=T, T=T, ny=2, nx=3, periodic=1, seas=P, ldc=C, D=D, row_of_t=ROWS, negate=0,
             bits=P, ldb=C,
             cell_of_point=P, C=C, basin=P, list_off=P, djdi=P, dist_m=P, north_m=P, east_m=P, n_entries=4,
             class_of_t=CLASSES, K=K, **d_out),
        [("short row_of_t", dict(row_of_t=short)), ("short class_of_t", dict(class_of_t=CLASSES[:-1])),
         ("both: short row_of_t and class_of_t", dict(row_of_t=short, class_of_t=CLASSES[:-1])),
         ("all: bad itemsize, short class_of_t, K", dict(itemsize=3, class_of_t=CLASSES[:-1], K=0)),
         ("both: bad itemsize and K", dict(itemsize=3, K=0)), ("K == 0", dict(K=0)), ("K above the cap", dict(K=dmax + 1)),
         ("C 2^31", dict(C=BIG)), ("ny above the cap", dict(ny=axis + 1)), ("nx above the cap", dict(nx=axis + 1)),
         ("ny == 0", dict(ny=0)),
         ("both: K and axis", dict(K=0, ny=axis + 1)), ("both: axis and ny == 0", dict(nx=axis + 1, ny=0)),
         ("t0 < 0", dict(t0=-1)),
         ("nt == 0", dict(nt=0)), ("nt past T", dict(t0=1)), ("C > ny * nx", dict(C=7, ldc=7, ldb=7, ldo=7)),
         ("ld < ny * nx", dict(ld=5)),
         ("ldb < C", dict(ldb=2)), ("D == 0", dict(D=0)), ("n_entries < 0", dict(n_entries=-1)),
         ("both: bad nt and ld", dict(nt=0, ld=5)),
         ("class >= K", dict(class_of_t=far)), ("class < -1", dict(class_of_t=CLASSES - 2)), ("row >= D", dict(D=3)),
         ("row < 0", dict(row_of_t=ROWS - 1)),
         ("both: class >= K and row >= D at one step", dict(class_of_t=np.full(T, K, np.int32), D=1)),
         ("both: row >= D at step 3, class >= K at step 5",
          dict(D=3, class_of_t=np.where(np.arange(T) == 5, K, 0).astype(np.int32))),
         ("both: bad ld and class >= K", dict(ld=5, class_of_t=far)), ("C == 0", dict(C=0)),
         ("both: row >= D and C == 0", dict(D=3, C=0)),
         ("both: row >= D and NULL", dict(D=3, ts=0)),
         ("no entries: the lists may be NULL, the outputs not",
          dict(n_entries=0, djdi=0, dist_m=0, north_m=0, east_m=0, n_days=0)),
         ("both: NULL buffer and list", dict(bits=0, djdi=0)), ("both: NULL list and output", dict(east_m=0, n_visited=0))],
        nulls=("ts", "seas", "bits", "cell_of_point", "list_off", "djdi", "dist_m", "north_m", "east_m", "n_days", "n_found",
               "sum_m",
               "sum_north_m", "sum_east_m", "max_m", "n_visited"), typed=True)
    return E


def covered(h, entries):
    """every public callable of the module is a case of the table, takes no device pointer, or is of the sharded path"""
    names = {n for n in dir(h) if not n.startswith("_") and callable(getattr(h, n)) and not isinstance(getattr(h, n), type)}
    have = {e.name for e in entries}
    assert not (have & NO_DEVICE_POINTER) and not (have & COMM) and not (NO_DEVICE_POINTER & COMM)
    missing = names - have - NO_DEVICE_POINTER - COMM
    assert not missing, f"bindings without a case in the table: {sorted(missing)}"
    gone = (have | NO_DEVICE_POINTER | COMM) - names
    assert not gone, f"the table names bindings the module does not have: {sorted(gone)}"


def replay(path):
    """the child: no device may be visible; then every case, in the table's order"""
    h = module()
    try:
        n = h.device_count()
    except h.HipError:
        n = 0
    if n:
        sys.exit(f"{n} device(s) visible: the refusal table runs without one")
    out = {}
    for entry in table(h):
        fn = getattr(h, entry.name)
        for case, kw in entry.calls():
            assert case not in out, case
            try:
                fn(*kw.values()) if entry.positional else fn(**kw)
                out[case] = "returned"
            except Exception as e:                      # noqa: BLE001 (the class is what the case records)
                out[case] = f"{type(e).__name__}: {e}"
    with open(path, "w") as f:
        json.dump(out, f)


def run_cases():
    """the table in a fresh child process that sees no device -> {case: outcome}"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--replay", path], env=env, check=True)
        with open(path) as f:
            return json.load(f)


def reached_the_runtime(outcome):
    return outcome.startswith(("HipError", "MemoryError"))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--replay":
        replay(sys.argv[2])
    else:
        h = module()
        covered(h, table(h))
        got = run_cases()
        bad = {k: v for k, v in got.items() if reached_the_runtime(v)}
        if bad:
            sys.exit("cases that reached the HIP runtime:\n" + "\n".join(f"  {k} -> {v}" for k, v in bad.items()))
        with open(FIXTURE, "w") as f:
            json.dump({"cases": got}, f, indent=0, sort_keys=True)
            f.write("\n")
        print(FIXTURE, len(got), "cases,", os.path.getsize(FIXTURE), "bytes")
