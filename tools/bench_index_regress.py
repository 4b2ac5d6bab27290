#!/usr/bin/env python3
"""index_regression()'s device pass on the resident float32 series of tools/bench_class_days.py: one JSON line.

    python tools/bench_index_regress.py [--cells 1036800] [--years 40] [--reps 10] [--blocks 256,512,4096,0] [--out FILE]

The series is generated on the device (the generator of bench.py).  Timed with HIP events around ONE C ABI call each,
median of --reps after a warm-up call, everything already on the device (the call pads and looks up its three host
tables in the content-keyed cache first, as every stage entry does: that host time is inside the interval):
  * xmhw_index_regress_accumulate_f32 with J = 1 / 8 / 32 predictors, K = 1 and the four seasons, a constant base
    (D = 1) and a climatology (D = 366); one more leg with 5 % scattered NaN (J = 8, seasons, D = 1): the deficit path;
  * the J = 32 seasons leg and the J = 8 one-class leg with every forced block length of --blocks (the integers must
    not change);
  * xmhw_class_sums_accumulate_f32 by year on the same series in the same run: the yardstick, the same frame without
    the products.
Reported with each leg: the ratio to the byte floor (the series once plus, for D = 366, a base row per step, at
6.3 TB/s, the measured copy rate), the ratio to the class-sums call and the multiply-adds per second (cells x steps x J
over the time).  numpy.linalg.lstsq per cell on --lstsq-cells cells of the same generator (J = 8 and an intercept) is
timed on the host and scaled to --cells."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
FIELDS = ("n", "sa", "saa", "n1", "saa1", "saz", "mz", "mzz")


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


def predictor_table(T, J, seed=3):
    """J standardised AR(1) columns in fixed point"""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(T, J))
    z = np.zeros((T, J))
    for t in range(1, T):
        z[t] = 0.95 * z[t - 1] + e[t]
    z = (z - z.mean(axis=0)) / z.std(axis=0)
    return np.rint(z * 65536.0).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1036800)
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", default="256,512,4096,0")
    ap.add_argument("--lstsq-cells", type=int, default=4096)
    ap.add_argument("--blocks-only", action="store_true", help="the forced block lengths alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_regress, hip_stress, require_gpu
    from xmhw_amd.days_by import class_labels
    require_gpu()
    h, hr, hs = hip(), hip_regress(), hip_stress()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    T, C = t.shape[0], a.cells
    year = class_labels("year", t)
    years = (year - year[0]).astype(np.int32)
    seasons = class_labels("season", t).astype(np.int32)
    classes = {"all": (np.zeros(T, np.int32), 1), "season": (seasons, 4)}
    zq = {J: predictor_table(T, J) for J in (1, 8, 32)}
    res = {"bench": "index_regress", "T": int(T), "cells": C, "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    d_ts = dev.DeviceBuffer(4 * T * C)
    h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, 0.0)
    h.stream_sync(0)
    d_cnt = dev.DeviceBuffer(8)

    # the yardstick: class sums by year on the same series
    d_n, d_s = dev.DeviceBuffer(4 * a.years * C), dev.DeviceBuffer(8 * a.years * C)
    hs.class_sums_init(a.years, C, d_n.ptr, d_s.ptr, C, d_cnt.ptr)
    sums = lambda: hs.class_sums_accumulate(d_ts.ptr, 4, T, C, C, 15.0, years, a.years, d_n.ptr, d_s.ptr, C, d_cnt.ptr)  # noqa: E731
    yard, every = median_ms(h, sums, a.reps)
    res["class_sums_years"] = {"K": a.years, "ms": round(yard, 3), "ms_all": every,
                               "over_floor": round(yard / (4 * T * C / HBM * 1e3), 2)}
    print(res["class_sums_years"], file=sys.stderr, flush=True)
    d_n.free()
    d_s.free()
    dump()

    bases = {1: dev.DeviceBuffer.from_array(np.full((1, C), 15.0)), 366: None}
    rows = {1: np.zeros(T, np.int32), 366: (np.arange(T) % 366).astype(np.int32)}

    def leg(J, cname, D, block=0, keep=False):
        kid, K = classes[cname]
        sizes = {k: (4 if k in ("n", "n1") else 8) * K * (J if k in ("saz", "mz", "mzz") else 1) * C for k in FIELDS}
        bufs = {k: dev.DeviceBuffer(nb) for k, nb in sizes.items()}
        ptrs = [bufs[k].ptr for k in FIELDS]
        hr.set_index_regress_block(block)
        hr.index_regress_init(K, J, C, *ptrs, C, d_cnt.ptr)
        call = lambda: hr.index_regress_accumulate(d_ts.ptr, 4, T, C, C, bases[D].ptr, C, D, rows[D], kid, K, zq[J], *ptrs, C,  # noqa: E731
                                                   d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        hr.index_regress_init(K, J, C, *ptrs, C, d_cnt.ptr)
        call()
        h.stream_sync(0)
        n = bufs["n"].to_array((K, C), np.int32)
        saz = bufs["saz"].to_array((K, J, C), np.int64) if keep else None
        n_range = int(d_cnt.to_array((1,), np.int64)[0])
        for b in bufs.values():
            b.free()
        floor = (4 + (8 if D > 1 else 0)) * T * C / HBM * 1e3
        return {"J": J, "classes": cname, "K": K, "D": D, "block": block, "ms": round(ms, 3), "ms_all": every,
                "byte_floor_ms": round(floor, 3), "over_floor": round(ms / floor, 2), "over_class_sums": round(ms / yard, 2),
                "mads_per_s": round(float(T) * C * J / (ms * 1e-3), -9), "valid_cell_steps": int(n.astype(np.int64).sum()),
                "n_range": n_range}, saz

    res["legs"] = []
    for D in (1, 366) if not a.blocks_only else ():
        if D == 366:
            bases[366] = dev.DeviceBuffer.from_array(np.full((366, C), 15.0) + 0.01 * np.arange(366)[:, None])
        for cname in ("all", "season"):
            for J in (1, 8, 32):
                r, _ = leg(J, cname, D)
                assert r["n_range"] == 0 and r["valid_cell_steps"] == T * C, r
                res["legs"].append(r)
                print(r, file=sys.stderr, flush=True)
                dump()
    if bases[366] is not None:
        bases[366].free()

    # forced block lengths at J = 32: same integers
    res["forced_blocks"] = []
    for J, cname in ((32, "season"), (8, "all")):
        ref = None
        for block in [int(b) for b in a.blocks.split(",")]:
            r, saz = leg(J, cname, 1, block=block, keep=True)
            ref = saz if ref is None else ref
            r["identical_integers"] = bool(np.array_equal(saz, ref))
            assert r["identical_integers"], f"block {block} changed the result"
            res["forced_blocks"].append(r)
            print(r, file=sys.stderr, flush=True)
        del ref, saz
    hr.set_index_regress_block(0)
    dump()

    if a.blocks_only:
        print(json.dumps(res))
        return dump()
    # the deficit path: 5 % scattered NaN
    h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, 0.05)
    h.stream_sync(0)
    r, _ = leg(8, "season", 1)
    r["nan_frac"] = 0.05
    r["invalid_share"] = round(1.0 - r["valid_cell_steps"] / (T * C), 4)
    res["nan_leg"] = r
    print(r, file=sys.stderr, flush=True)
    dump()
    for b in (d_ts, d_cnt, bases[1]):
        b.free()

    # the host route: numpy.linalg.lstsq per cell on a few cells of the same generator
    n = a.lstsq_cells
    if n > 0:
        d_small = dev.DeviceBuffer(4 * T * n)
        h.synth_sst(d_small.ptr, 4, T, n, n, 0, 7, 0.0)
        h.stream_sync(0)
        x = d_small.to_array((T, n), np.float32).astype(np.float64) - 15.0
        d_small.free()
        A = np.concatenate([np.ones((T, 1)), zq[8] / 65536.0], axis=1)
        t0 = time.perf_counter()
        for c in range(n):
            np.linalg.lstsq(A, x[:, c], rcond=None)
        s = time.perf_counter() - t0
        j8 = next(r for r in res["legs"] if r["J"] == 8 and r["D"] == 1 and r["classes"] == "all")
        res["lstsq_host"] = {"cells": n, "J": 8, "seconds": round(s, 3), "scaled_to_cells_s": round(s * C / n, 1),
                             "over_device": round(s * C / n / (j8["ms"] * 1e-3), 0)}
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
