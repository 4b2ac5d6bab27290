#!/usr/bin/env python3
"""coarsen()'s device pass on the resident float32 series of tools/bench_spatial_correlation.py, an uncompacted
ny x 1440 grid: one JSON line.

    python tools/bench_coarsen.py [--ny 720] [--nx 1440] [--years 40] [--reps 3] [--chunks 0,4,128,1024] [--out FILE]

The series is generated on the device (the generator of bench.py).  Timed with HIP events around ONE C ABI call each,
median of --reps after a warm-up call, everything already on the device (the call looks up its window table in the
content-keyed cache first, as every stage entry does: that host time is inside the interval):
  * xmhw_coarsen_f32 with the factors (fy, fx, len) = (2, 2, 1), (4, 4, 1), (3, 3, 1) -- the run-time column loop --,
    (1, 1, 30) and (4, 4, 5), the optional outputs not written;
  * (2, 2, 1) on a series with 5 % scattered NaN, and in float64 (on the first half of the steps: the float64 series of
    all of them would not fit beside the float32 one);
  * the wide loads against loads of one sample and against the column loop on the same input, (2, 2, 1) and (4, 4, 1)
    (the bits of the first and the last 32 windows must not change);
  * (2, 2, 1) with every forced chunk of --chunks windows (the bits must not change): what the automatic rule of
    csrc/stage_blocks.h rests on;
  * the comparator, in the same run on the same series: xmhw_region_accumulate_f32 with one region, the only device
    route to a spatial mean before coarsen().
Reported with each leg: the ratio to the byte floor at 6.3 TB/s -- every sample of a window once, the weights once and
every output entry once -- and the ratio to the comparator."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
CLASSES = ("column loop", "fx 1", "fx 2, one sample a load", "fx 2, wide", "fx 4, one sample a load", "fx 4, wide")


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
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunks", default="0,4,128,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_coarsen, require_gpu
    require_gpu()
    h, hc = hip(), hip_coarsen()
    T = int(np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]").shape[0])
    ny, nx = a.ny, a.nx
    N = ny * nx
    res = {"bench": "coarsen", "T": T, "ny": ny, "nx": nx, "points": N, "hbm_bytes_per_s": HBM, "reps": a.reps}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    def series(seed, isz=4, steps=T, nan_frac=0.0):
        d = dev.DeviceBuffer(isz * steps * N)
        h.synth_sst(d.ptr, isz, steps, N, N, 0, seed, nan_frac)
        h.stream_sync(0)
        return d

    wi = np.rint(np.repeat(np.cos(np.deg2rad(np.linspace(-89.875, 89.875, ny))), nx) * (1 << 24)).astype(np.int32)
    d_wi = dev.DeviceBuffer.from_array(wi)
    d_cnt = dev.DeviceBuffer.from_array(np.zeros(2, np.int64))

    def leg(d_x, fy, fx, length, isz=4, steps=T, variant=0, chunk=0, what="coarsen", keep=False):
        win = np.arange(0, steps - steps % length + 1, length, dtype=np.int32)
        S, ncy, ncx = win.shape[0] - 1, ny // fy, nx // fx
        cells = ncy * ncx
        d_out = dev.DeviceBuffer(isz * S * cells)
        hc.set_coarsen_variant(variant)
        hc.set_coarsen_chunk(chunk)
        klass = hc.coarsen_class(d_x.ptr, d_wi.ptr, N, nx, isz, fx)
        call = lambda: hc.coarsen(d_x.ptr, isz, steps, N, ny, nx, fy, fx, ncy, ncx, d_wi.ptr, 15.0, 32768, win,  # noqa: E731
                                  d_out.ptr, cells, 0, 0, d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        out = None
        if keep:                                      # the first and the last 32 windows: 2 x 32 x cells values
            rows = min(32, S)
            out = np.empty((2, rows, cells), np.float32 if isz == 4 else np.float64)
            h.memcpy_d2h(out[0], d_out.ptr)
            h.memcpy_d2h(out[1], d_out.ptr + isz * (S - rows) * cells)
        d_out.free()
        hc.set_coarsen_variant(0)
        hc.set_coarsen_chunk(0)
        read, written = isz * int(win[-1]) * ncy * fy * ncx * fx + 4 * N, isz * S * cells
        floor = (read + written) / HBM * 1e3
        return {"what": what, "factors": [fy, fx, length], "dtype": f"float{8 * isz}", "steps": steps, "windows": S, "cells": cells,
                "instantiation": CLASSES[klass], "variant": variant, "chunk": chunk, "ms": round(ms, 3), "ms_all": every,
                "bytes_read": read, "bytes_written": written, "byte_floor_ms": round(floor, 3),
                "over_floor": round(ms / floor, 2), "read_TB_per_s": round(read / (ms * 1e-3) / 1e12, 3)}, out

    def record(r, where="legs"):
        res.setdefault(where, []).append(r)
        print(r, file=sys.stderr, flush=True)
        dump()

    d_x = series(7)
    # the comparator: one region over the whole grid, (T, 1, 3) int64 sums
    d_region = dev.DeviceBuffer.from_array(np.zeros(N, np.int32))
    d_wi64 = dev.DeviceBuffer.from_array(wi.astype(np.int64))
    d_acc = dev.DeviceBuffer.from_array(np.zeros((T, 1, 3), np.int64))
    ms, every = median_ms(h, lambda: h.region_accumulate(d_x.ptr, 4, T, N, N, 15.0, d_wi64.ptr, d_region.ptr, 1, d_acc.ptr,
                                                         d_cnt.ptr + 8), a.reps)
    floor = (4 * T * N + 12 * N) / HBM * 1e3
    comparator = {"what": "region_accumulate, one region: the comparator", "ms": round(ms, 3), "ms_all": every,
                  "byte_floor_ms": round(floor, 3), "over_floor": round(ms / floor, 2)}
    record(comparator, "comparator")
    for b in (d_region, d_wi64, d_acc):
        b.free()

    def over(r):
        r["over_comparator"] = round(r["ms"] / comparator["ms"], 3)
        return r

    for fy, fx, length in ((2, 2, 1), (4, 4, 1), (3, 3, 1), (1, 1, 30), (4, 4, 5)):
        record(over(leg(d_x, fy, fx, length)[0]))
    assert int(d_cnt.to_array((2,), np.int64)[0]) == 0, "samples out of range"
    # wide loads against loads of one sample against the column loop: same bits
    for fy, fx in ((2, 2), (4, 4)):
        ref = None
        for variant in (0, 1, 2):
            r, out = leg(d_x, fy, fx, 1, variant=variant, keep=True, what="coarsen, forced instantiation")
            ref = out if ref is None else ref
            r["identical_bits"] = bool(np.array_equal(out.view(np.uint32), ref.view(np.uint32)))
            assert r["identical_bits"], f"variant {variant} changed the result"
            record(over(r), "instantiations")
        del ref, out
    # forced chunks of windows: same bits
    ref = None
    for chunk in [int(c) for c in a.chunks.split(",")]:
        r, out = leg(d_x, 2, 2, 1, chunk=chunk, keep=True, what="coarsen, forced chunk of windows")
        ref = out if ref is None else ref
        r["identical_bits"] = bool(np.array_equal(out.view(np.uint32), ref.view(np.uint32)))
        assert r["identical_bits"], f"chunk {chunk} changed the result"
        record(over(r), "forced_chunks")
    del ref, out
    d_x.free()
    d_gaps = series(7, nan_frac=0.05)
    record(over(leg(d_gaps, 2, 2, 1, what="coarsen, 5 % scattered NaN")[0]))
    d_gaps.free()
    half = T // 2
    d_x64 = series(7, isz=8, steps=half)
    record(leg(d_x64, 2, 2, 1, isz=8, steps=half, what="coarsen, float64, the first half of the steps")[0])
    d_x64.free()
    for b in (d_wi, d_cnt):
        b.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
