#!/usr/bin/env python3
"""heat_stress()'s device stages on the resident float32 series of tools/bench_class_days.py: one JSON line.

    python tools/bench_heat_stress.py [--cells 1036800] [--years 40] [--reps 5] [--blocks 256,1024,4096,0] [--out FILE]

The series is generated on the device (the generator of bench.py).  Timed with HIP events around ONE C ABI call each,
median of --reps after a warm-up call, everything already on the device:
  * xmhw_class_sums_accumulate_f32 by calendar month (K = 12), the pass behind maximum_monthly_mean();
  * xmhw_heat_stress_accumulate_f32 with the Coral Reef Watch defaults (W = 84, h0 = 1.0 above the MMM of the first
    pass, levels 4 and 8 degree heating weeks, one snapshot at the last step) by year (K = --years), with the automatic
    block length and with every forced block length of --blocks (the spread is the evidence for the automatic choice);
  * xmhw_class_days_accumulate_f32 by year on the same series in the same run -- the yardstick of the neighbouring
    stages -- with the raw climatologies of the threshold kernel and the bits of xmhw_exceed_bits on the same cells.
Reported with each: the ratio to the byte floor (the series once plus the outputs, at 6.3 TB/s, the measured copy rate)
and the ratio to the class-days call.  The integers of the forced block lengths must equal those of the automatic one."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--cells", type=int, default=1036800)
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", default="256,1024,4096,0")
    ap.add_argument("--no-yardstick", action="store_true", help="skip the class-days call and its climatologies")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_stress, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.days_by import class_labels
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.heat_stress import levels_q
    require_gpu()
    h, hs = hip(), hip_stress()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    T, C = t.shape[0], a.cells
    year = class_labels("year", t)
    years = (year - year[0]).astype(np.int32)
    months = (class_labels("month", t) - 1).astype(np.int32)
    res = {"bench": "heat_stress", "T": int(T), "cells": C, "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    d_ts = dev.DeviceBuffer(4 * T * C)
    h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, 0.0)
    h.stream_sync(0)

    # class sums by month -> the MMM
    d_n, d_s, d_cnt = dev.DeviceBuffer(4 * 12 * C), dev.DeviceBuffer(8 * 12 * C), dev.DeviceBuffer(8)
    sums = lambda: hs.class_sums_accumulate(d_ts.ptr, 4, T, C, C, 0.0, months, 12, d_n.ptr, d_s.ptr, C, d_cnt.ptr)  # noqa: E731
    ms, every = median_ms(h, sums, a.reps)
    hs.class_sums_init(12, C, d_n.ptr, d_s.ptr, C, d_cnt.ptr)
    sums()
    h.stream_sync(0)
    n, s = d_n.to_array((12, C), np.int32), d_s.to_array((12, C), np.int64)
    assert int(d_cnt.to_array((1,), np.int64)[0]) == 0 and (n == np.bincount(months, minlength=12)[:, None]).all()
    mmm = (s.astype(np.float64) / n.astype(np.float64) / 65536.0).max(axis=0)
    floor = (4 * T * C + 12 * 12 * C) / HBM * 1e3
    res["class_sums_months"] = {"K": 12, "ms": round(ms, 3), "ms_all": every, "byte_floor_ms": round(floor, 3),
                                "over_floor": round(ms / floor, 2)}
    print(res["class_sums_months"], file=sys.stderr, flush=True)
    dump()

    # heat stress by year, Coral Reef Watch defaults
    K, W, level_q, at = a.years, 84, levels_q((4.0, 8.0), 7.0), np.array([T - 1], np.int32)
    rows = np.zeros(T, np.int32)
    d_base = dev.DeviceBuffer.from_array(mmm[None])
    bufs = {k: dev.DeviceBuffer(nb) for k, nb in (("counts", 4 * 8 * K * C), ("hsum", 8 * K * C), ("key", 8 * K * C),
                                                  ("snap", 4 * C), ("pq", 4 * K * C), ("pt", 4 * K * C))}
    stress = lambda: hs.heat_stress_accumulate(d_ts.ptr, 4, T, C, C, d_base.ptr, C, 1, rows, 0, W, 1.0, years, K, level_q, at,  # noqa: E731
                                               bufs["counts"].ptr, bufs["hsum"].ptr, bufs["key"].ptr, bufs["snap"].ptr, C,
                                               d_cnt.ptr)
    floor = (4 * T * C + (4 * 8 + 8 + 8) * K * C + 4 * C) / HBM * 1e3

    def one(block):
        hs.set_heat_stress_block(block)
        ms, every = median_ms(h, stress, a.reps)
        hs.heat_stress_init(K, C, bufs["counts"].ptr, bufs["hsum"].ptr, bufs["key"].ptr, C, d_cnt.ptr)
        stress()
        hs.heat_stress_finish(K, C, bufs["key"].ptr, bufs["pq"].ptr, bufs["pt"].ptr, C)
        h.stream_sync(0)
        out = (bufs["counts"].to_array((K, 8, C), np.int32), bufs["hsum"].to_array((K, C), np.int64),
               bufs["pq"].to_array((K, C), np.int32), bufs["pt"].to_array((K, C), np.int32), bufs["snap"].to_array((1, C), np.int32))
        assert int(d_cnt.to_array((1,), np.int64)[0]) == 0
        return {"block": block, "ms": round(ms, 3), "ms_all": every, "over_floor": round(ms / floor, 2)}, out

    auto, ref = one(0)
    hot = int(ref[0][:, 1].astype(np.int64).sum())
    res["heat_stress_years"] = dict(auto, K=K, W=W, byte_floor_ms=round(floor, 3), hot_cell_days=hot,
                                    hot_share=round(hot / (T * C), 4), cells_with_stress=int((ref[2].max(axis=0) > 0).sum()),
                                    peak_dhw_max=round(float(ref[2].max()) / (7 * 65536.0), 2),
                                    alert1_cell_days=int(ref[0][:, 2].astype(np.int64).sum()))
    print(res["heat_stress_years"], file=sys.stderr, flush=True)
    dump()
    res["forced_blocks"] = []
    for block in [int(b) for b in a.blocks.split(",") if int(b) > 0]:
        r, out = one(block)
        r["class_sums_months_ms"] = round(median_ms(h, sums, a.reps)[0], 3)
        r["identical_integers"] = all(np.array_equal(x, y) for x, y in zip(out, ref))
        assert r["identical_integers"], f"block {block} changed the result"
        res["forced_blocks"].append(r)
        print(r, file=sys.stderr, flush=True)
    hs.set_heat_stress_block(0)
    del ref, out
    for b in list(bufs.values()) + [d_base, d_n, d_s]:
        b.free()
    dump()

    # the yardstick: class days by year on the same series
    if not a.no_yardstick:
        doy = add_doy(t)
        plan = dev.Plan(doy, 5)
        D = plan.D
        _, _, _, rows = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((D, 1)), np.zeros((D, 1)), doy, np.unique(doy))
        d_th, d_se = dev.DeviceBuffer(8 * D * C), dev.DeviceBuffer(8 * D * C)
        dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
        d_bits = dev.DeviceBuffer(8 * ((T + 63) // 64) * C)
        h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C)
        d_days, d_isum, d_imax = dev.DeviceBuffer(4 * 6 * K * C), dev.DeviceBuffer(8 * K * C), dev.DeviceBuffer(8 * K * C)
        h.class_days_init(K, C, d_days.ptr, d_isum.ptr, d_imax.ptr, C, d_cnt.ptr)
        h.stream_sync(0)
        ms, every = median_ms(h, lambda: h.class_days_accumulate(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C, rows, 0, d_bits.ptr, C,
                                                                 5, 1, 2, years, K, d_days.ptr, d_isum.ptr, d_imax.ptr, C, d_cnt.ptr),
                              a.reps)
        res["class_days_years"] = {"K": K, "ms": round(ms, 3), "ms_all": every}
        res["class_sums_months"]["over_class_days"] = round(res["class_sums_months"]["ms"] / ms, 2)
        res["heat_stress_years"]["over_class_days"] = round(res["heat_stress_years"]["ms"] / ms, 2)
        for b in (d_th, d_se, d_bits, d_days, d_isum, d_imax):
            b.free()
        plan.destroy()
    for b in (d_ts, d_cnt):
        b.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
