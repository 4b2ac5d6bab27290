#!/usr/bin/env python3
"""mhw_days_by()'s device stage on the resident float32 series of tools/bench_coverage.py: one JSON line.

    python tools/bench_class_days.py [--cells 518400,1036800] [--years 40] [--reps 10] [--route-cells 4096] [--out FILE]

The series is generated on the device (the generator of bench.py), the climatologies are the raw threshold / seasonal
mean of the threshold kernel on the same cells, the exceedance bits those of xmhw_exceed_bits.  Per cell count and class
pattern -- one class, calendar months (K = 12), the 40 years (K = 40) and labels that change every step (t % 7, K = 7:
the flush-per-step worst case) -- the device time of xmhw_class_days_accumulate_f32 (in-event bitmap + reduction) is
taken with HIP events around the C ABI call, median of --reps after a warm-up call, everything already on the device.
Alongside, in the same run and on the same buffers: xmhw_coverage_accumulate_f32 with one region (it reads the same
bytes, with a reduction across lanes in place of the register runs), the byte floor (one read of the series plus the
in-event bitmap at 6.3 TB/s, the measured copy rate), and the numpy route to the same day counts --
detect_cells(..., intermediate=True) and a masked reduction of `cats` / `events` per class -- timed on --route-cells
cells and scaled linearly; those cells double as the spot check: both routes must give identical integers.
A 65,536-cell slab is timed with the automatic block length and with one block over all of T (block 1,000,000): the
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
    from xmhw_amd.days_by import class_days_cells, class_labels
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
    year = class_labels("year", t)
    patterns = [("one_class", np.zeros(T, np.int32), 1),
                ("months", (class_labels("month", t) - 1).astype(np.int32), 12),
                ("years", (year - year[0]).astype(np.int32), a.years),
                ("every_step", (np.arange(T) % 7).astype(np.int32), 7)]
    res = {"bench": "mhw_days_by", "T": int(T), "D": int(D), "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps,
           "cases": [], "small_slab": []}

    def on_device(C, seed=7):
        d_ts = dev.DeviceBuffer(4 * T * C)
        h.synth_sst(d_ts.ptr, 4, T, C, C, 0, seed, 0.0)
        d_th, d_se = dev.DeviceBuffer(8 * D * C), dev.DeviceBuffer(8 * D * C)
        dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
        h.stream_sync(0)
        return d_ts, d_th, d_se

    def time_pattern(C, bufs, classes, K):
        d_ts, d_th, d_se, d_bits = bufs
        d_days, d_isum, d_imax, d_cnt = (dev.DeviceBuffer(4 * 6 * K * C), dev.DeviceBuffer(8 * K * C),
                                         dev.DeviceBuffer(8 * K * C), dev.DeviceBuffer(8))
        h.class_days_init(K, C, d_days.ptr, d_isum.ptr, d_imax.ptr, C, d_cnt.ptr)
        ms, every = median_ms(h, lambda: h.class_days_accumulate(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, rows, 0,
                                                                 d_bits.ptr, C, 5, 1, 2, classes, K, d_days.ptr, d_isum.ptr,
                                                                 d_imax.ptr, C, d_cnt.ptr), a.reps)
        days = d_days.to_array((K, 6, C), np.int32)
        n_range = int(d_cnt.to_array((1,), np.int64)[0])
        for b in (d_days, d_isum, d_imax, d_cnt):
            b.free()
        return ms, every, int(days[:, 4].astype(np.int64).sum()) // (a.reps + 1), n_range     # every call accumulated

    for C in [int(c) for c in a.cells.split(",")]:
        d_ts, d_th, d_se = on_device(C)
        d_bits = dev.DeviceBuffer(8 * W * C)
        h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C)
        h.stream_sync(0)
        floor_ms = (4 * T * C + T * C / 8) / HBM * 1e3
        d_wq, d_reg = dev.DeviceBuffer.from_array(np.ones(C, np.int64)), dev.DeviceBuffer.from_array(np.zeros(C, np.int32))
        d_c, d_a = dev.DeviceBuffer(8 * T * 5), dev.DeviceBuffer(8 * T * 5)
        h.memset(d_c.ptr, 0, 8 * T * 5)
        h.memset(d_a.ptr, 0, 8 * T * 5)
        cov_ms, cov_all = median_ms(h, lambda: h.coverage_accumulate(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, rows, 0,
                                                                     d_bits.ptr, C, 5, 1, 2, d_wq.ptr, d_reg.ptr, 1, d_c.ptr,
                                                                     d_a.ptr), a.reps)
        for b in (d_wq, d_reg, d_c, d_a):
            b.free()
        for name, classes, K in patterns:
            ms, every, event_days, n_range = time_pattern(C, (d_ts, d_th, d_se, d_bits), classes, K)
            res["cases"].append({
                "cells": C, "classes": name, "K": K, "class_days_accumulate_ms": round(ms, 3),
                "class_days_accumulate_ms_all": every, "coverage_accumulate_R1_ms": round(cov_ms, 3),
                "coverage_accumulate_R1_ms_all": cov_all, "over_coverage_accumulate": round(ms / cov_ms, 2),
                "byte_floor_ms": round(floor_ms, 3), "over_floor": round(ms / floor_ms, 2),
                "in_event_cell_days": event_days, "in_event_share": round(event_days / (T * C), 4), "n_range": n_range})
            print(res["cases"][-1], file=sys.stderr, flush=True)
        for b in (d_ts, d_th, d_se, d_bits):
            b.free()

    # a slab smaller than the full grid: the automatic block length against one block over all of T
    C = 65536
    d_ts, d_th, d_se = on_device(C)
    d_bits = dev.DeviceBuffer(8 * W * C)
    h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C)
    h.stream_sync(0)
    try:
        for name, classes, K in patterns[1::2]:
            for block in (0, 1000000):
                h.set_class_days_block(block)
                ms, every, _, _ = time_pattern(C, (d_ts, d_th, d_se, d_bits), classes, K)
                res["small_slab"].append({"cells": C, "classes": name, "block_steps": block,
                                          "class_days_accumulate_ms": round(ms, 3), "class_days_accumulate_ms_all": every})
                print(res["small_slab"][-1], file=sys.stderr, flush=True)
    finally:
        h.set_class_days_block(0)
    for b in (d_ts, d_th, d_se, d_bits):
        b.free()

    # the numpy route to the day counts, on a cell count a host holds; the same cells through the stage
    n = a.route_cells
    d_ts, d_th, d_se = on_device(n)
    ts, th, se = d_ts.to_array((T, n), np.float32), d_th.to_array((D, n), np.float64), d_se.to_array((D, n), np.float64)
    for b in (d_ts, d_th, d_se):
        b.free()
    _, classes, K = patterns[1]
    t0 = time.perf_counter()
    r = detect_cells(ts, se, th, doy, doys, intermediate=True)
    t_detect = time.perf_counter() - t0
    t0 = time.perf_counter()
    cats, ev = r["inter"]["cats"], ~np.isnan(r["inter"]["events"])
    states = [cats == 1, cats == 2, cats == 3, cats >= 4, ev]
    want = np.stack([np.stack([s[classes == k].sum(axis=0) for s in states]) for k in range(K)]).astype(np.int32)
    t_numpy = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = class_days_cells(ts, se, th, doy, doys, classes, K)
    t_stage = time.perf_counter() - t0
    assert np.array_equal(got[0][:, :5], want) and want[:, 4].sum() > 0
    res["numpy_route"] = {"cells": n, "classes": "months", "detect_cells_intermediate_s": round(t_detect, 3),
                          "numpy_reduction_s": round(t_numpy, 3), "total_s": round(t_detect + t_numpy, 3),
                          "class_days_cells_wall_s": round(t_stage, 3), "identical_integers": True,
                          "in_event_cell_days": int(want[:, 4].sum())}
    for c in res["cases"]:
        scaled = (t_detect + t_numpy) * c["cells"] / n
        c["numpy_route_scaled_s"] = round(scaled, 2)
        c["numpy_route_over_accumulate"] = round(scaled * 1e3 / c["class_days_accumulate_ms"], 1)
    plan.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
