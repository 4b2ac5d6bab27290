#!/usr/bin/env python3
"""region_series()'s device stage on a synthetic 40-year daily series: one JSON line.

    python tools/bench_region_series.py [--cells 518400,1036800] [--years 40] [--reps 10] [--route-cells 4096] [--out FILE]

The float32 series is generated on the device (the generator of bench.py), with and without 5 % scattered NaN.  Per
cell count and region layout -- one region; 64 latitude-longitude boxes; 64 labels scattered per cell -- the device
time of the one C ABI call xmhw_region_accumulate_f32 is taken with HIP events, median of reps after a warm-up call,
everything already on the device, once per wave-sum variant (0: one wave sum per step, 1: the sums of 8 steps together,
the default); both variants must leave identical accumulators.  Each figure is reported
(a) as a multiple of its byte floor: one read of the series at 6.3 TB/s (HBM, measured copy rate: DESIGN.md 5),
(b) next to xmhw_coverage_accumulate_f32 on the same series, regions and weights in the same run (the existing
    cross-cell pass over the same bytes; its exceedance bits are made once, outside the timing), and
(c) against the route it replaces: the series on the host and a numpy weighted sum per region, timed here on
    --route-cells cells and scaled linearly to the cell count.  Those cells double as the spot check: the device
    integers must equal numpy's rint / int64 sums exactly."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
NLON = 1440


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


def layouts(C, rng):
    """(name, R, region ids): cells are rows of NLON longitudes, as a global grid is stacked"""
    lat, lon = np.arange(C) // NLON, np.arange(C) % NLON
    nlat = (C + NLON - 1) // NLON
    boxes = ((lat * 8 // nlat) * 8 + lon * 8 // NLON).astype(np.int32)
    return (("one_region", 1, np.zeros(C, np.int32)), ("boxes_8x8", 64, boxes),
            ("scattered_64", 64, rng.integers(0, 64, C).astype(np.int32)))


def waves_by_path(reg):
    """how many waves of 64 consecutive cells hold 1, 2..4 and more regions (paths A, B, C of the kernel)"""
    n = reg.shape[0] // 64 * 64
    r = np.sort(reg[:n].reshape(-1, 64), axis=1)
    k = 1 + (np.diff(r, axis=1) != 0).sum(axis=1)
    return {"A": int((k == 1).sum()), "B": int(((k > 1) & (k <= 4)).sum()), "C": int((k > 4).sum())}


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
    from xmhw_amd.detect_front import _check_inputs
    from xmhw_amd.region_series import region_cells, weight_bits
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
    res = {"bench": "region_series", "T": int(T), "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps, "cases": []}
    rng = np.random.default_rng(3)
    try:
        for C in [int(c) for c in a.cells.split(",")]:
            ib = weight_bits(C)
            wi = rng.integers(0, (1 << ib) + 1, C, dtype=np.int64)
            d_wi = dev.DeviceBuffer.from_array(wi)
            d_wq = dev.DeviceBuffer.from_array(wi << (31 - ib))              # coverage's weights: the same, at 31 bits
            floor_ms = 4 * T * C / HBM * 1e3
            for nan_frac in (0.0, 0.05):
                d_ts = dev.DeviceBuffer(4 * T * C)
                h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, nan_frac)
                d_th, d_se = dev.DeviceBuffer(8 * D * C), dev.DeviceBuffer(8 * D * C)
                dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
                d_bits = dev.DeviceBuffer(8 * W * C)
                h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, D, rows, 0, d_bits.ptr, C)
                h.stream_sync(0)
                for name, R, reg in layouts(C, rng):
                    d_reg = dev.DeviceBuffer.from_array(reg)
                    case = {"cells": C, "nan_frac": nan_frac, "regions": name, "R": R, "weight_bits": ib,
                            "waves_by_path": waves_by_path(reg), "byte_floor_ms": round(floor_ms, 3)}
                    accs = []
                    for variant, label in ((0, "per_step"), (1, "blocked8")):
                        h.set_region_wave_sum(variant)
                        d_acc, d_nr = dev.DeviceBuffer(8 * T * R * 3), dev.DeviceBuffer(8)
                        h.memset(d_acc.ptr, 0, 8 * T * R * 3)
                        h.memset(d_nr.ptr, 0, 8)
                        ms, every = median_ms(h, lambda: h.region_accumulate(d_ts.ptr, 4, T, C, C, 0.0, d_wi.ptr, d_reg.ptr,
                                                                             R, d_acc.ptr, d_nr.ptr), a.reps)
                        accs.append(d_acc.to_array((T, R, 3), np.int64))
                        assert int(d_nr.to_array((1,), np.int64)[0]) == 0
                        case[f"region_accumulate_ms_{label}"] = round(ms, 3)
                        case[f"region_accumulate_ms_{label}_all"] = every
                        case[f"over_floor_{label}"] = round(ms / floor_ms, 2)
                        case[f"tb_per_s_{label}"] = round(4 * T * C / ms / 1e9, 2)
                        d_acc.free()
                        d_nr.free()
                    h.set_region_wave_sum(1)
                    assert np.array_equal(accs[0], accs[1]) and accs[0][..., 0].sum() > 0
                    valid = accs[0][..., 0].sum() // (a.reps + 1)             # every call accumulated
                    case["valid_share"] = round(float(valid) / (T * C), 4)
                    d_c, d_a = dev.DeviceBuffer(8 * T * R * 5), dev.DeviceBuffer(8 * T * R * 5)
                    h.memset(d_c.ptr, 0, 8 * T * R * 5)
                    h.memset(d_a.ptr, 0, 8 * T * R * 5)
                    cov_ms, cov_all = median_ms(h, lambda: h.coverage_accumulate(d_ts.ptr, 4, T, C, C, d_se.ptr, d_th.ptr, C,
                                                                                 rows, 0, d_bits.ptr, C, 5, 1, 2, d_wq.ptr,
                                                                                 d_reg.ptr, R, d_c.ptr, d_a.ptr), a.reps)
                    case["coverage_accumulate_ms"] = round(cov_ms, 3)
                    case["coverage_accumulate_ms_all"] = cov_all
                    res["cases"].append(case)
                    print(case, file=sys.stderr, flush=True)
                    for b in (d_reg, d_c, d_a):
                        b.free()
                for b in (d_ts, d_th, d_se, d_bits):
                    b.free()
            d_wi.free()
            d_wq.free()
    finally:
        h.set_region_wave_sum(1)
        plan.destroy()

    # (c) the route this replaces, on a cell count a host holds; the same cells through the device stage
    n = a.route_cells
    d_ts = dev.DeviceBuffer(4 * T * n)
    h.synth_sst(d_ts.ptr, 4, T, n, n, 0, 7, 0.05)
    h.stream_sync(0)
    ts = d_ts.to_array((T, n), np.float32)
    d_ts.free()
    reg = (np.arange(n) * 64 // n).astype(np.int32)
    ib = weight_bits(n)
    w = rng.random(n)
    wi = np.rint(w / w.max() * (1 << ib)).astype(np.int64)
    t0 = time.perf_counter()
    mean = np.empty((T, 64))
    for r in range(64):
        sel = reg == r
        x = ts[:, sel].astype(np.float64)
        ok = ~np.isnan(x)
        mean[:, r] = np.where(ok, x * w[sel], 0.0).sum(axis=1) / (ok * w[sel]).sum(axis=1)
    t_numpy = time.perf_counter() - t0
    t0 = time.perf_counter()
    got, n_range = region_cells(ts, wi, reg, 64)
    t_dev = time.perf_counter() - t0
    xq = np.rint(np.where(np.isnan(ts), 0.0, ts.astype(np.float64)) * 65536.0).astype(np.int64)
    ok = (~np.isnan(ts)).astype(np.int64)
    want = np.stack([np.stack([ok[:, reg == r].sum(axis=1), (ok[:, reg == r] * wi[reg == r]).sum(axis=1),
                               (xq[:, reg == r] * wi[reg == r]).sum(axis=1)], axis=-1) for r in range(64)], axis=1)
    assert n_range == 0 and np.array_equal(got, want)
    dmean = got[..., 2] / (got[..., 1] * 65536.0)
    res["numpy_route"] = {"cells": n, "regions": 64, "numpy_weighted_sums_s": round(t_numpy, 3),
                          "region_cells_wall_s": round(t_dev, 3), "identical_integers": True,
                          "max_abs_mean_difference": float(np.nanmax(np.abs(dmean - mean)))}
    for c in res["cases"]:
        scaled = t_numpy * c["cells"] / n
        c["numpy_route_scaled_s"] = round(scaled, 2)
        c["numpy_route_over_stage"] = round(scaled * 1e3 / c["region_accumulate_ms_blocked8"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
