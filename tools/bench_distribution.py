#!/usr/bin/env python3
"""anomaly_distribution()'s device passes on the resident float32 series of tools/bench_class_days.py: one JSON line.

    python tools/bench_distribution.py [--cells 1036800] [--years 40] [--reps 5] [--blocks 256,512,4096,0] [--out FILE]

The series is generated on the device (the generator of bench.py).  Timed with HIP events around ONE C ABI call each,
median of --reps after a warm-up call, everything already on the device (the call looks up its two host tables in the
content-keyed cache first, as every stage entry does: that host time is inside the interval):
  * xmhw_distribution_accumulate_f32 with B = 64 / 128 / 256 bins (32 / 64 / 128 KB of LDS per workgroup) for one class, by
    calendar month, by year and with labels that change every step; a constant base (one row) and, for 128 bins, a
    366-row base;
  * 128 bins by month on a series with 5 % scattered NaN;
  * one class with 128 and 256 bins and every forced block length of --blocks and one block (the integers must not
    change): what the automatic rule of csrc/stage_blocks.h rests on;
  * xmhw_distribution_finish alone with 5 and with 16 quantiles (and 2 levels), by month, 128 bins;
  * xmhw_class_sums_accumulate_f32 by year on the same series in the same run: the yardstick, a pass that reads every
    sample.
Reported with each leg: the ratio to the class-sums call and to the byte floor at 6.3 TB/s -- every sample and base row
once and the 68 bytes of sums and extremes of every (class, cell) entry; the histogram rows a flush touches are not in the
floor --, and the valid samples per second."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
ACC = (("hist", 4), ("n", 4), ("s1", 8), ("s2", 8), ("s3", 16), ("s4", 16), ("kmin", 8), ("kmax", 8))
ONE = 65536


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
    ap.add_argument("--blocks", default="256,512,4096,0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_distribution, hip_stress, require_gpu
    from xmhw_amd.days_by import class_labels
    require_gpu()
    h, hd, hs = hip(), hip_distribution(), hip_stress()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    T, C = t.shape[0], a.cells
    year = class_labels("year", t)
    years = (year - year[0]).astype(np.int32)
    classes = {"all": (np.zeros(T, np.int32), 1), "month": ((class_labels("month", t) - 1).astype(np.int32), 12),
               "year": (years, a.years), "every step": ((np.arange(T) % 3).astype(np.int32), 3)}
    res = {"bench": "anomaly_distribution", "T": int(T), "cells": C, "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    def series(seed, nan_frac=0.0):
        d = dev.DeviceBuffer(4 * T * C)
        h.synth_sst(d.ptr, 4, T, C, C, 0, seed, nan_frac)
        h.stream_sync(0)
        return d

    d_x = series(7)
    d_cnt = dev.DeviceBuffer(16)

    # the yardstick: class sums by year on the same series
    d_n, d_s = dev.DeviceBuffer(4 * a.years * C), dev.DeviceBuffer(8 * a.years * C)
    hs.class_sums_init(a.years, C, d_n.ptr, d_s.ptr, C, d_cnt.ptr)
    sums = lambda: hs.class_sums_accumulate(d_x.ptr, 4, T, C, C, 15.0, years, a.years, d_n.ptr, d_s.ptr, C, d_cnt.ptr)  # noqa: E731
    yard, every = median_ms(h, sums, a.reps)
    res["class_sums_years"] = {"K": a.years, "ms": round(yard, 3), "ms_all": every,
                               "over_floor": round(yard / (4 * T * C / HBM * 1e3), 2)}
    print(res["class_sums_years"], file=sys.stderr, flush=True)
    d_n.free()
    d_s.free()
    dump()

    bases = {1: dev.DeviceBuffer.from_array(np.full((1, C), 15.0)), 366: None}
    rows = {1: np.zeros(T, np.int32), 366: (np.arange(T) % 366).astype(np.int32)}

    def bins(B):
        return -32 * ONE, 64 * ONE // B, B           # -32 .. 32 around the base of 15

    def leg(d_a, B, cname, Dr, block=0, keep=False, what=None, finish=()):
        """one accumulate call; ``finish``: the numbers of quantiles to time the finish pass with afterwards"""
        kid, K = classes[cname]
        bufs = {k: dev.DeviceBuffer(size * K * (B + 2 if k == "hist" else 1) * C) for k, size in ACC}
        ptrs = [bufs[k].ptr for k, _ in ACC]
        hd.set_distribution_block(block)
        hd.distribution_init(K, B, C, *ptrs, C, d_cnt.ptr)
        call = lambda: hd.distribution_accumulate(d_a.ptr, 4, T, C, C, bases[Dr].ptr, C, Dr, rows[Dr], 0, kid, K, *bins(B),  # noqa: E731
                                                  *ptrs, C, d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        hd.distribution_init(K, B, C, *ptrs, C, d_cnt.ptr)
        call()
        h.stream_sync(0)
        n = bufs["n"].to_array((K, C), np.int32)
        out = (n, bufs["s2"].to_array((K, C), np.int64), bufs["s4"].to_array((K, 2, C), np.int64)) if keep else None
        n_range = int(d_cnt.to_array((1,), np.int64)[0])
        samples, touched = int(n.astype(np.int64).sum()), int(np.count_nonzero(n))
        floor = (T * C * (4 + (8 if Dr > 1 else 0)) + 68 * touched) / HBM * 1e3
        r = {"what": what or "accumulate", "bins": B, "lds_kb": 32 if B <= 64 else 64 if B <= 128 else 128, "classes": cname,
             "K": K, "base_rows": Dr, "block": block, "ms": round(ms, 3), "ms_all": every, "byte_floor_ms": round(floor, 3),
             "over_floor": round(ms / floor, 2), "over_class_sums": round(ms / yard, 2), "samples": samples,
             "samples_per_s": round(samples / (ms * 1e-3), -8), "n_range": n_range}
        fins = []
        for P in finish:
            q = [dev.DeviceBuffer(4 * K * P * C) for _ in range(3)] + [dev.DeviceBuffer(4 * K * 2 * C)]
            p_q = np.rint(np.linspace(0.01, 0.99, P) * 4294967296.0).astype(np.uint64)
            edge = np.array([B // 2, 3 * B // 4], np.int32)
            # (the keys are turned to float64 at the first call; the later calls time the same walk)
            fin = lambda: hd.distribution_finish(K, B, C, bufs["hist"].ptr, bufs["n"].ptr, bufs["kmin"].ptr, bufs["kmax"].ptr,  # noqa: E731
                                                 p_q, edge, *(b.ptr for b in q), C)
            fms, fevery = median_ms(h, fin, a.reps)
            ffloor = 4 * K * C * (B + 2 + 1 + 4 + 3 * P + 2) / HBM * 1e3
            fins.append({"what": "finish", "bins": B, "classes": cname, "K": K, "quantiles": P, "levels": 2, "ms": round(fms, 3),
                         "ms_all": fevery, "byte_floor_ms": round(ffloor, 3), "over_floor": round(fms / ffloor, 2)})
            for b in q:
                b.free()
        for b in bufs.values():
            b.free()
        return r, out, fins

    res["legs"], res["finish"] = [], []

    def record(r, where="legs"):
        res[where].append(r)
        print(r, file=sys.stderr, flush=True)
        dump()

    for B in (64, 128, 256):
        for cname in classes:
            r, _, fins = leg(d_x, B, cname, 1, finish=(5, 16) if (B, cname) == (128, "month") else ())
            assert r["samples"] > 0, r
            record(r)
            for f in fins:
                record(f, "finish")
    bases[366] = dev.DeviceBuffer.from_array(np.full((366, C), 15.0) + 0.01 * np.arange(366)[:, None])
    for cname in classes:
        record(leg(d_x, 128, cname, 366)[0])
    bases[366].free()
    d_gaps = series(7, 0.05)
    record(leg(d_gaps, 128, "month", 1, what="accumulate, 5 % scattered NaN")[0])
    d_gaps.free()

    # forced block lengths: same integers
    res["forced_blocks"] = []
    for B in (128, 256):
        ref = None
        for block in [int(b) for b in a.blocks.split(",")] + [T]:
            r, out, _ = leg(d_x, B, "all", 1, block=block, keep=True)
            ref = out if ref is None else ref
            r["identical_integers"] = bool(all(np.array_equal(u, v) for u, v in zip(out, ref)))
            assert r["identical_integers"], f"block {block} changed the result"
            record(r, "forced_blocks")
        del ref, out
    hd.set_distribution_block(0)
    for b in (d_x, d_cnt, bases[1]):
        b.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
