#!/usr/bin/env python3
"""The two kernels of detrend() on a synthetic series resident on the device: one JSON document.

    python tools/bench_detrend.py [--cells 518400,1036800] [--steps 14610] [--reps 10] [--sample 4096] [--out FILE]

For every grid size, gap-free and with 5 % NaN, and (order, harmonics) = (1, 0), (1, 2), (3, 3): HIP events around
xmhw_series_fit_f32 and xmhw_series_remove_f32 (the C ABI calls, series already on the device), median of ``reps``
after a warm-up.  Each stage is reported against its byte floor -- fit: T*C*4 bytes read, remove: 2*T*C*4 bytes read
and written, at the 6.29 TB/s copy rate of DESIGN.md section 5.  For scale, numpy.linalg.lstsq on ``sample`` cells
of the same series on the host, scaled per cell (the route this replaces, without its PCIe copies)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
CONFIGS = ((1, 0), (1, 2), (3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="518400,1036800")
    ap.add_argument("--steps", type=int, default=14610)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.detrend import DetrendSpec
    from xmhw_amd.device import DeviceBuffer
    require_gpu()
    h = hip()
    T = a.steps
    time_axis = np.datetime64("1982-01-01") + np.arange(T).astype("timedelta64[D]")
    specs = {cfg: DetrendSpec(time_axis, *cfg) for cfg in CONFIGS}
    e0, e1, e2 = h.event_create(), h.event_create(), h.event_create()
    results = []
    sample_host = None
    for C in [int(c) for c in a.cells.split(",")]:
        d_ts = DeviceBuffer(4 * T * C)
        d_coef = DeviceBuffer(8 * 10 * C)
        d_nv = DeviceBuffer(4 * C)
        for nan_frac in (0.0, 0.05):
            for cfg in CONFIGS:
                spec = specs[cfg]
                d_b, _ = spec._upload()
                h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, nan_frac)     # a fresh series: the removal works in place
                h.stream_sync(0)
                if sample_host is None and nan_frac == 0.05:
                    n = min(a.sample, C)
                    sample_host = np.empty((T, n), dtype=np.float32)
                    full = np.empty((T, C), dtype=np.float32) if C <= 65536 else None
                    if full is not None:
                        h.memcpy_d2h(full, d_ts.ptr)
                        sample_host[:] = full[:, :n]
                    else:
                        d_idx = DeviceBuffer.from_array(np.arange(n, dtype=np.int64))
                        d_s = DeviceBuffer(4 * T * n)
                        h.gather_cells(d_ts.ptr, 4, T, C, d_idx.ptr, n, d_s.ptr, n)
                        h.stream_sync(0)
                        sample_host[:] = d_s.to_array((T, n), np.float32)
                        d_idx.free(); d_s.free()
                fit_ms, rem_ms = [], []
                for _ in range(a.reps + 1):
                    h.event_record(e0, 0)
                    h.series_fit(d_ts.ptr, 4, T, C, C, d_b.ptr, spec.P, 0, spec.min_valid, d_coef.ptr, C, d_nv.ptr)
                    h.event_record(e1, 0)
                    h.series_remove(d_ts.ptr, 4, T, C, C, d_b.ptr, spec.P, spec.R, d_coef.ptr, C)
                    h.event_record(e2, 0)
                    h.stream_sync(0)
                    fit_ms.append(h.event_elapsed_ms(e0, e1))
                    rem_ms.append(h.event_elapsed_ms(e1, e2))
                nfail = int(np.isnan(d_coef.to_array((C,), np.float64)).sum())
                f, r = float(np.median(fit_ms[1:])), float(np.median(rem_ms[1:]))
                fit_floor, rem_floor = 4.0 * T * C / COPY_RATE * 1e3, 8.0 * T * C / COPY_RATE * 1e3
                row = {"cells": C, "steps": T, "nan_frac": nan_frac, "order": cfg[0], "harmonics": cfg[1], "terms": spec.P,
                       "fit_ms": round(f, 3), "fit_ms_all": [round(v, 3) for v in fit_ms[1:]],
                       "fit_floor_ms": round(fit_floor, 3), "fit_x_floor": round(f / fit_floor, 2),
                       "remove_ms": round(r, 3), "remove_ms_all": [round(v, 3) for v in rem_ms[1:]],
                       "remove_floor_ms": round(rem_floor, 3), "remove_x_floor": round(r / rem_floor, 2),
                       "failed_cells": nfail}
                results.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        for b in (d_ts, d_coef, d_nv):
            b.free()
    for e in (e0, e1, e2):
        h.event_destroy(e)
    # the host route on a sample of cells of the 5 % NaN series
    cpu = []
    for cfg in CONFIGS:
        spec = specs[cfg]
        B = spec.basis
        t0 = time.perf_counter()
        for c in range(sample_host.shape[1]):
            y = sample_host[:, c].astype(np.float64)
            ok = ~np.isnan(y)
            beta = np.linalg.lstsq(B[ok], y[ok], rcond=None)[0]
            _ = y - B[:, :spec.R] @ beta[:spec.R]
        dt = time.perf_counter() - t0
        cpu.append({"order": cfg[0], "harmonics": cfg[1], "sample_cells": int(sample_host.shape[1]),
                    "lstsq_us_per_cell": round(dt / sample_host.shape[1] * 1e6, 1)})
    for row in results:
        us = next(c["lstsq_us_per_cell"] for c in cpu if (c["order"], c["harmonics"]) == (row["order"], row["harmonics"]))
        row["cpu_lstsq_s_scaled"] = round(us * 1e-6 * row["cells"], 1)
        row["cpu_lstsq_over_gpu"] = round(us * 1e-6 * row["cells"] / ((row["fit_ms"] + row["remove_ms"]) * 1e-3), 0)
    for s in specs.values():
        s.free()
    doc = {"bench": "detrend", "copy_rate_bytes_per_s": COPY_RATE, "reps": a.reps, "results": results, "cpu": cpu}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
