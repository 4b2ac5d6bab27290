#!/usr/bin/env python3
"""mhw_cooccurrence()'s device stage on the tables of two resident detections: one JSON line.

    python tools/bench_cooccurrence.py [--cells 518400,1036800] [--years 40] [--reps 10] [--route-cells 4096] [--out FILE]

Two float32 series are generated on the device (the generator of bench.py, two seeds); each goes through the threshold
kernel and the device detect() stage (xmhw_exceed_bits, xmhw_events_from_bits, xmhw_event_stats_sparse), and only the
index_start / index_end columns and the offsets of its table stay resident.  Per cell count the two xmhw_event_table_bits
calls are timed together, and xmhw_cooccur_accumulate for three class patterns -- one class, calendar months (K = 12),
labels that change every step (t % 7, K = 7: the flush-per-segment worst case) -- times L = 1, 8 and 64 lags (leads
0 .. L-1), with HIP events around the C ABI calls, median of --reps after a warm-up call, everything already on the
device.  Alongside, in the same run: the byte floor (the tables read once, the bitmaps written once and read once per
group of 8 lags, at 6.3 TB/s, the measured copy rate), and the numpy route to the same integers --
detect_cells(..., intermediate=True) twice and masked sums of the two dense (T, cells) event masks per class and lag --
timed on --route-cells cells and scaled linearly; those cells double as the spot check: both routes must give identical
integers.  A 65,536-cell slab is timed with the automatic block and with one block over all words (block 1,000,000): the
case that decides whether the time axis is split."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
SEEDS = (7, 8)


def median_ms(h, fn, reps):
    e0, e1 = h.event_create(), h.event_create()
    out = []
    for _ in range(reps + 1):
        h.event_record(e0, 0)
        fn()
        h.event_record(e1, 0)
        h.stream_sync(0)
        out.append(h.event_elapsed_ms(e0, e1))
    h.event_destroy(e0)
    h.event_destroy(e1)
    return float(np.median(out[1:])), [round(v, 3) for v in out[1:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="518400,1036800")
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route-cells", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.cooccurrence import cooccur_tables
    from xmhw_amd.days_by import class_labels
    from xmhw_amd.detect import EVENT_COLUMNS
    from xmhw_amd.detect_front import _check_inputs, detect_cells
    require_gpu()
    h = hip()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    doy = add_doy(t)
    T = t.shape[0]
    W = (T + 63) // 64
    plan = dev.Plan(doy, 5)
    D = plan.D
    doys = np.unique(doy)
    _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((D, 1)), np.zeros((D, 1)), doy, doys)
    patterns = [("one_class", np.zeros(T, np.int32), 1),
                ("months", (class_labels("month", t) - 1).astype(np.int32), 12),
                ("every_step", (np.arange(T) % 7).astype(np.int32), 7)]
    lag_lists = [np.arange(L, dtype=np.int32) for L in (1, 8, 64)]
    res = {"bench": "mhw_cooccurrence", "T": int(T), "W": int(W), "hbm_bytes_per_s": HBM, "reps": a.reps, "seeds": list(SEEDS),
           "cases": [], "rasteriser": [], "small_slab": []}

    def series(C, seed):
        d_ts = dev.DeviceBuffer(4 * T * C)
        h.synth_sst(d_ts.ptr, 4, T, C, C, 0, seed, 0.0)
        d_th, d_se = dev.DeviceBuffer(8 * D * C), dev.DeviceBuffer(8 * D * C)
        dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
        h.stream_sync(0)
        return d_ts, d_th, d_se

    def table_on_device(C, seed):
        """the device detect() stage on one series; returns the resident (start, end, offsets, cell) and the row count"""
        d_ts, d_th, d_se = series(C, seed)
        with dev.DeviceScope() as s:
            for b in (d_ts, d_th, d_se):
                s.adopt(b)
            d_bits, d_n = s.alloc(8 * W * C), s.alloc(4 * C)
            d_off = dev.DeviceBuffer(8 * (C + 1))
            h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C)
            h.events_from_bits(d_bits.ptr, T, C, C, 5, 1, 2, 0, d_n.ptr, 0)
            h.offsets_from_counts(d_n.ptr, C, d_off.ptr)
            h.stream_sync(0)
            n = int(d_off.to_array((C + 1,), np.int64)[-1])
            ncol = h.EVENT_COLUMNS
            d_tab = s.alloc(8 * max(n, 1) * ncol)
            h.events_from_bits(d_bits.ptr, T, C, C, 5, 1, 2, d_off.ptr, 0, d_tab.ptr)
            h.event_stats_sparse(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, rows, 0, n, d_tab.ptr)
            h.stream_sync(0)
            start, end = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
            step = 1 << 20
            chunk = np.empty((step, ncol), dtype=np.float64)
            for r0 in range(0, n, step):
                m = min(step, n - r0)
                h.memcpy_d2h(chunk[:m], d_tab.ptr + 8 * ncol * r0)
                start[r0:r0 + m], end[r0:r0 + m] = chunk[:m, 1], chunk[:m, 2]
        return (dev.DeviceBuffer.from_array(start), dev.DeviceBuffer.from_array(end), d_off,
                dev.DeviceBuffer.from_array(np.arange(C, dtype=np.int64))), n

    def resident(C):
        """both tables and both bitmaps of C cells on the device, and the time of the two rasteriser calls"""
        tabs, n_rows = zip(*(table_on_device(C, seed) for seed in SEEDS))
        bits = [dev.DeviceBuffer(8 * W * C) for _ in SEEDS]

        def rasterise():
            for (d_start, d_end, d_off, d_cell), d_bits in zip(tabs, bits):
                h.event_table_bits(d_start.ptr, d_end.ptr, d_off.ptr, d_cell.ptr, C, T, d_bits.ptr, C)
        ms, every = median_ms(h, rasterise, a.reps)
        floor = (sum(n_rows) * 8 + 2 * C * 16 + 2 * 8 * W * C) / HBM * 1e3
        for tab in tabs:
            for b in tab:
                b.free()
        return bits, n_rows, {"cells": C, "rows": list(n_rows), "event_table_bits_x2_ms": round(ms, 3),
                              "event_table_bits_x2_ms_all": every, "byte_floor_ms": round(floor, 4),
                              "over_floor": round(ms / floor, 2)}

    def time_accumulate(C, bits, classes, K, lags):
        L = lags.shape[0]
        d_counts = dev.DeviceBuffer(4 * 4 * K * L * C)
        h.cooccur_init(K, L, C, d_counts.ptr, C)
        ms, every = median_ms(h, lambda: h.cooccur_accumulate(bits[0].ptr, C, bits[1].ptr, C, T, C, classes, K, lags,
                                                              d_counts.ptr, C), a.reps)
        h.cooccur_init(K, L, C, d_counts.ptr, C)
        h.cooccur_accumulate(bits[0].ptr, C, bits[1].ptr, C, T, C, classes, K, lags, d_counts.ptr, C)
        h.stream_sync(0)
        both = int(d_counts.to_array((C,), np.int32).astype(np.int64).sum())       # class 0, the first lag, `both`
        d_counts.free()
        return ms, every, both

    for C in [int(c) for c in a.cells.split(",")]:
        bits, n_rows, ras = resident(C)
        res["rasteriser"].append(ras)
        print(ras, file=sys.stderr, flush=True)
        for name, classes, K in patterns:
            for lags in lag_lists:
                L = int(lags.shape[0])
                ms, every, both = time_accumulate(C, bits, classes, K, lags)
                floor_ms = 2 * 8 * W * C * ((L + 7) // 8) / HBM * 1e3
                res["cases"].append({"cells": C, "classes": name, "K": K, "L": L, "cooccur_accumulate_ms": round(ms, 3),
                                     "cooccur_accumulate_ms_all": every, "byte_floor_ms": round(floor_ms, 4),
                                     "over_floor": round(ms / floor_ms, 2), "joint_cell_days_class0_lag0": both})
                print(res["cases"][-1], file=sys.stderr, flush=True)
        for b in bits:
            b.free()

    # a slab smaller than the full grid: the automatic block against one block over all words
    C = 65536
    bits, _, _ = resident(C)
    try:
        for name, classes, K in patterns[1:]:
            for block in (0, 1000000):
                h.set_cooccur_block(block)
                ms, every, _ = time_accumulate(C, bits, classes, K, lag_lists[1])
                res["small_slab"].append({"cells": C, "classes": name, "L": 8, "block_words": block,
                                          "cooccur_accumulate_ms": round(ms, 3), "cooccur_accumulate_ms_all": every})
                print(res["small_slab"][-1], file=sys.stderr, flush=True)
    finally:
        h.set_cooccur_block(0)
    for b in bits:
        b.free()

    # the numpy route to the same integers, on a cell count a host holds; the same cells through the stage
    n = a.route_cells
    _, classes, K = patterns[1]
    lags = lag_lists[1]
    t_detect, masks, views = 0.0, [], []
    for seed in SEEDS:
        d_ts, d_th, d_se = series(n, seed)
        ts, th, se = d_ts.to_array((T, n), np.float32), d_th.to_array((D, n), np.float64), d_se.to_array((D, n), np.float64)
        for b in (d_ts, d_th, d_se):
            b.free()
        t0 = time.perf_counter()
        r = detect_cells(ts, se, th, doy, doys, intermediate=True)
        t_detect += time.perf_counter() - t0
        masks.append(~np.isnan(r["inter"]["events"]))
        tab = r["table"]
        views.append(dict(n=tab.shape[0], C=n, offsets=np.ascontiguousarray(r["offsets"], dtype=np.int64),
                          start=tab[:, EVENT_COLUMNS.index("index_start")].astype(np.int32),
                          end=tab[:, EVENT_COLUMNS.index("index_end")].astype(np.int32)))
    t0 = time.perf_counter()
    A, B = masks
    want = np.zeros((K, lags.shape[0], 3, n), dtype=np.int32)
    for i, lag in enumerate(int(v) for v in lags):
        hi = T - lag
        a_, b_, k_ = A[:hi], B[lag:], classes[:hi]
        for k in range(K):
            sel = k_ == k
            want[k, i, 0] = (a_[sel] & b_[sel]).sum(axis=0)
            want[k, i, 1] = (a_[sel] & ~b_[sel]).sum(axis=0)
            want[k, i, 2] = (~a_[sel] & b_[sel]).sum(axis=0)
    t_numpy = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = cooccur_tables(views[0], views[1], np.arange(n), np.arange(n), T, classes, K, lags)
    t_stage = time.perf_counter() - t0
    assert np.array_equal(got[:, :, :3], want) and want[:, :, 0].sum() > 0
    res["numpy_route"] = {"cells": n, "classes": "months", "L": 8, "detect_cells_intermediate_x2_s": round(t_detect, 3),
                          "numpy_reduction_s": round(t_numpy, 3), "total_s": round(t_detect + t_numpy, 3),
                          "cooccur_tables_wall_s": round(t_stage, 3), "identical_integers": True,
                          "joint_cell_days": int(want[:, :, 0].sum())}
    ras_ms = {r["cells"]: r["event_table_bits_x2_ms"] for r in res["rasteriser"]}
    for c in res["cases"]:
        if c["classes"] == "months" and c["L"] == 8:
            scaled = (t_detect + t_numpy) * c["cells"] / n
            c["numpy_route_scaled_s"] = round(scaled, 2)
            c["numpy_route_over_device"] = round(scaled * 1e3 / (c["cooccur_accumulate_ms"] + ras_ms[c["cells"]]), 1)
    plan.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
