#!/usr/bin/env python3
"""lag_correlation()'s device pass on the resident float32 series of tools/bench_class_days.py: one JSON line.

    python tools/bench_lag_correlation.py [--cells 1036800] [--years 40] [--reps 10] [--blocks 256,512,4096,0] [--out FILE]

The series are generated on the device (the generator of bench.py; the second field is the same generator with another
seed).  Timed with HIP events around ONE C ABI call each, median of --reps after a warm-up call, everything already on the
device (the call looks up its two host tables in the content-keyed cache first, as every stage entry does: that host time
is inside the interval):
  * xmhw_lag_corr_accumulate_f32 with y = x (autocorrelation) and 1 / 8 / 32 / 64 lags, and with a second field and 32
    lags; one class and the four seasons; constant bases (one row) and 366-row bases;
  * the autocorrelation with 8 lags by season on a series with 5 % scattered NaN;
  * the 32- and 64-lag autocorrelation of one class with every forced block length of --blocks (the integers must not change):
    what the automatic rule of csrc/stage_blocks.h rests on;
  * xmhw_class_sums_accumulate_f32 by year on the same series in the same run: the yardstick, a pass that reads every
    sample.
Reported with each leg: the ratio to the class-sums call and to the byte floor at 6.3 TB/s -- every series and base row
once and the 44 bytes of every accumulator entry that is touched --, the valid pairs per second and, in ``per_lag``, the
time per further lag between the legs of 1 and 64 lags, which goes next to the 0.955 ms per predictor of
index_regression()."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
FIELDS = ("n", "sx", "sy", "sxx", "syy", "sxy")


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", default="256,512,4096,0")
    ap.add_argument("--blocks-only", action="store_true", help="the forced block lengths alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_lagcorr, hip_stress, require_gpu
    from xmhw_amd.days_by import class_labels
    require_gpu()
    h, hl, hs = hip(), hip_lagcorr(), hip_stress()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    T, C = t.shape[0], a.cells
    year = class_labels("year", t)
    years = (year - year[0]).astype(np.int32)
    classes = {"all": (np.zeros(T, np.int32), 1), "season": (class_labels("season", t).astype(np.int32), 4)}
    res = {"bench": "lag_correlation", "T": int(T), "cells": C, "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps}

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

    def leg(d_a, d_b, nlags, cname, Dr, block=0, keep=False, what=None):
        """one accumulate call on (d_a, d_b); d_b None: the autocorrelation, the same pointer twice"""
        L = nlags - 1
        kid, K = classes[cname]
        bufs = {k: dev.DeviceBuffer((4 if k == "n" else 8) * K * nlags * C) for k in FIELDS}
        ptrs = [bufs[k].ptr for k in FIELDS]
        two = d_b is not None
        y = d_b if two else d_a
        hl.set_lag_corr_block(block)
        hl.lag_corr_init(K, L, C, *ptrs, C, d_cnt.ptr)
        call = lambda: hl.lag_corr_accumulate(d_a.ptr, C, y.ptr, C, 4, T, C, bases[Dr].ptr, C, bases[Dr].ptr, C, Dr, rows[Dr],  # noqa: E731
                                              0, 0, kid, K, L, *ptrs, C, d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        hl.lag_corr_init(K, L, C, *ptrs, C, d_cnt.ptr)
        call()
        h.stream_sync(0)
        n = bufs["n"].to_array((K, nlags, C), np.int32)
        out = tuple([n] + [bufs[k].to_array((K, nlags, C), np.int64) for k in FIELDS[1:]]) if keep else None
        n_range = [int(v) for v in d_cnt.to_array((2,), np.int64)]
        for b in bufs.values():
            b.free()
        pairs, touched = int(n.astype(np.int64).sum()), int(np.count_nonzero(n))
        floor = ((2 if two else 1) * T * C * (4 + (8 if Dr > 1 else 0)) + 44 * touched) / HBM * 1e3
        return {"what": what or ("two fields" if two else "autocorrelation"), "lags": nlags, "classes": cname, "K": K,
                "base_rows": Dr, "block": block, "ms": round(ms, 3), "ms_all": every, "byte_floor_ms": round(floor, 3),
                "over_floor": round(ms / floor, 2), "over_class_sums": round(ms / yard, 2), "pairs": pairs,
                "pairs_per_s": round(pairs / (ms * 1e-3), -8), "entries_touched": touched, "n_range": n_range}, out

    res["legs"] = []

    def record(r):
        res["legs"].append(r)
        print(r, file=sys.stderr, flush=True)
        dump()

    if not a.blocks_only:
        for Dr in (1, 366):
            if Dr == 366:
                bases[366] = dev.DeviceBuffer.from_array(np.full((366, C), 15.0) + 0.01 * np.arange(366)[:, None])
            for cname in ("all", "season"):
                for nlags in (1, 8, 32, 64):
                    r, _ = leg(d_x, None, nlags, cname, Dr)
                    assert r["n_range"] == [0, 0] and r["pairs"] > 0, r
                    record(r)
        # the time per further lag, per class pattern and base
        res["per_lag"] = []
        for Dr in (1, 366):
            for cname in ("all", "season"):
                ms = {r["lags"]: r["ms"] for r in res["legs"] if r["classes"] == cname and r["base_rows"] == Dr}
                res["per_lag"].append({"classes": cname, "base_rows": Dr,
                                       "ms_per_further_lag_1_to_64": round((ms[64] - ms[1]) / 63.0, 4),
                                       "ms_per_further_lag_32_to_64": round((ms[64] - ms[32]) / 32.0, 4),
                                       "index_regress_ms_per_predictor": 0.955})
        print(res["per_lag"], file=sys.stderr, flush=True)
        # two fields, 32 lags
        d_y = series(11)
        for Dr in (1, 366):
            for cname in ("all", "season"):
                r, _ = leg(d_x, d_y, 32, cname, Dr)
                assert r["n_range"] == [0, 0] and r["pairs"] > 0, r
                record(r)
        d_y.free()
        # 5 % scattered NaN
        d_gaps = series(7, 0.05)
        r, _ = leg(d_gaps, None, 8, "season", 1, what="autocorrelation, 5 % scattered NaN")
        record(r)
        r, _ = leg(d_gaps, None, 64, "season", 1, what="autocorrelation, 5 % scattered NaN")
        record(r)
        d_gaps.free()
    if bases[366] is not None:
        bases[366].free()

    # forced block lengths: same integers
    res["forced_blocks"] = []
    for nlags in (32, 64):
        ref = None
        for block in [int(b) for b in a.blocks.split(",")] + [T]:
            r, out = leg(d_x, None, nlags, "all", 1, block=block, keep=True)
            ref = out if ref is None else ref
            r["identical_integers"] = bool(all(np.array_equal(u, v) for u, v in zip(out, ref)))
            assert r["identical_integers"], f"block {block} changed the result"
            res["forced_blocks"].append(r)
            print(r, file=sys.stderr, flush=True)
            dump()
        del ref, out
    hl.set_lag_corr_block(0)
    for b in (d_x, d_cnt, bases[1]):
        b.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
