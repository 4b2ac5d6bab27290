#!/usr/bin/env python3
"""mhw_coverage()'s device stage on a synthetic 40-year daily series: one JSON line.

    python tools/bench_coverage.py [--cells 518400,1036800] [--years 40] [--reps 5] [--route-cells 4096] [--out FILE]

The float32 series is generated on the device (the generator of bench.py), the climatologies are the raw
threshold / seasonal mean of the threshold kernel on the same cells.  Per cell count and region layout (R = 1;
R = 64, ids scattered per cell) the device time of xmhw_exceed_bits (the stage shared with detect()) and of
xmhw_coverage_accumulate (in-event bitmap + reduction) is taken with HIP events around the C ABI calls, median of
reps after a warm-up call, everything already on the device.  Each figure is reported against
(a) its byte floor: one read of the series plus the exceedance bits at 6.3 TB/s (HBM, measured copy rate), and
(b) the only route to the same numbers before mhw_coverage(): detect_cells(..., intermediate=True) and a numpy
    reduction of `cats` / `events`, timed here on --route-cells cells (what a host holds comfortably: eleven
    (T, C) float64 arrays come back) and scaled linearly to the cell count for the comparison.
The table-only detect() device stage (bits, run count + prefix sum, table fill + statistics; HIP events, without the
allocation and the read-back of the table) is timed on the same buffers, so that
the added cost of the coverage reduction over it can be read off.  The route-(b) cells double as the spot check:
both routes must give identical integers."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route-cells", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.coverage import coverage_cells
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
    res = {"bench": "mhw_coverage", "T": int(T), "D": int(D), "dtype": "float32", "hbm_bytes_per_s": HBM, "cases": []}

    def on_device(C, seed=7):
        d_ts = dev.DeviceBuffer(4 * T * C)
        h.synth_sst(d_ts.ptr, 4, T, C, C, 0, seed, 0.0)
        d_th, d_se = dev.DeviceBuffer(8 * D * C), dev.DeviceBuffer(8 * D * C)
        dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
        h.stream_sync(0)
        return d_ts, d_th, d_se

    for C in [int(c) for c in a.cells.split(",")]:
        d_ts, d_th, d_se = on_device(C)
        d_bits = dev.DeviceBuffer(8 * W * C)
        bits_ms, bits_all = median_ms(h, lambda: h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C),
                                      a.reps)
        # table-only detect() device stage on the same buffers and bits: count + prefix sum, then fill + statistics
        d_n, d_off = dev.DeviceBuffer(4 * C), dev.DeviceBuffer(8 * (C + 1))

        def count():
            h.events_from_bits(d_bits.ptr, T, C, C, 5, 1, 2, 0, d_n.ptr, 0)
            h.offsets_from_counts(d_n.ptr, C, d_off.ptr)
        count_ms, _ = median_ms(h, count, a.reps)
        total = np.empty(1, dtype=np.int64)
        h.memcpy_d2h(total, d_off.ptr + 8 * C)
        n_events = int(total[0])
        d_tab = dev.DeviceBuffer(8 * max(n_events, 1) * h.EVENT_COLUMNS)

        def fill():
            h.events_from_bits(d_bits.ptr, T, C, C, 5, 1, 2, d_off.ptr, 0, d_tab.ptr)
            h.event_stats_sparse(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, rows, 0, n_events, d_tab.ptr)
        fill_ms, _ = median_ms(h, fill, a.reps)
        table_ms = bits_ms + count_ms + fill_ms
        for b in (d_n, d_off, d_tab):
            b.free()
        floor_ms = (4 * T * C + T * C / 8) / HBM * 1e3
        rng = np.random.default_rng(3)
        for R, name in ((1, "R1"), (64, "R64_scattered")):
            reg = np.zeros(C, np.int32) if R == 1 else rng.integers(0, R, C).astype(np.int32)
            wq = rng.integers(0, (1 << 31) + 1, C, dtype=np.int64)
            d_wq, d_reg = dev.DeviceBuffer.from_array(wq), dev.DeviceBuffer.from_array(reg)
            d_c, d_a = dev.DeviceBuffer(8 * T * R * 5), dev.DeviceBuffer(8 * T * R * 5)
            h.memset(d_c.ptr, 0, 8 * T * R * 5)
            h.memset(d_a.ptr, 0, 8 * T * R * 5)
            cov_ms, cov_all = median_ms(h, lambda: h.coverage_accumulate(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, rows, 0,
                                                                         d_bits.ptr, C, 5, 1, 2, d_wq.ptr, d_reg.ptr, R,
                                                                         d_c.ptr, d_a.ptr), a.reps)
            cells = d_c.to_array((T, R, 5), np.int64) // (a.reps + 1)            # every call accumulated
            res["cases"].append({
                "cells": C, "regions": name, "exceed_bits_ms": round(bits_ms, 3), "exceed_bits_ms_all": bits_all,
                "coverage_accumulate_ms": round(cov_ms, 3), "coverage_accumulate_ms_all": cov_all,
                "coverage_stage_ms": round(bits_ms + cov_ms, 3), "byte_floor_ms": round(floor_ms, 3),
                "stage_over_floor": round((bits_ms + cov_ms) / floor_ms, 2),
                "table_only_detect_stage_ms": round(table_ms, 3), "n_events": n_events,
                "accumulate_over_table_only_detect": round(cov_ms / table_ms, 2),
                "in_event_cell_days": int(cells[..., 4].sum()), "in_event_share": round(float(cells[..., 4].sum()) / (T * C), 4),
                "max_cells_in_event_on_one_day": int(cells[..., 4].sum(axis=1).max())})
            print(res["cases"][-1], file=sys.stderr, flush=True)
            for b in (d_wq, d_reg, d_c, d_a):
                b.free()
        for b in (d_ts, d_th, d_se, d_bits):
            b.free()

    # (b) the route this replaces, on a cell count a host holds; the same cells through mhw_coverage's stage
    n = a.route_cells
    d_ts, d_th, d_se = on_device(n)
    ts, th, se = d_ts.to_array((T, n), np.float32), d_th.to_array((D, n), np.float64), d_se.to_array((D, n), np.float64)
    for b in (d_ts, d_th, d_se):
        b.free()
    t0 = time.perf_counter()
    r = detect_cells(ts, se, th, doy, doys, intermediate=True)
    t_detect = time.perf_counter() - t0
    t0 = time.perf_counter()
    cats, ev = r["inter"]["cats"], ~np.isnan(r["inter"]["events"])
    want = np.stack([(cats == 1).sum(axis=1), (cats == 2).sum(axis=1), (cats == 3).sum(axis=1), (cats >= 4).sum(axis=1),
                     ev.sum(axis=1)], axis=-1).astype(np.int64)
    t_numpy = time.perf_counter() - t0
    t0 = time.perf_counter()
    got, _ = coverage_cells(ts, se, th, doy, doys, np.ones(n, np.int64), np.zeros(n, np.int32), 1)
    t_cov = time.perf_counter() - t0
    assert np.array_equal(got[:, 0], want) and want[:, 4].sum() > 0
    res["per_step_route"] = {"cells": n, "detect_cells_intermediate_s": round(t_detect, 3), "numpy_reduction_s": round(t_numpy, 3),
                             "total_s": round(t_detect + t_numpy, 3), "coverage_cells_wall_s": round(t_cov, 3),
                             "identical_integers": True, "in_event_cell_days": int(want[:, 4].sum())}
    for c in res["cases"]:
        scaled = (t_detect + t_numpy) * c["cells"] / n
        c["per_step_route_scaled_s"] = round(scaled, 2)
        c["per_step_route_over_stage"] = round(scaled * 1e3 / c["coverage_stage_ms"], 1)
    plan.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
