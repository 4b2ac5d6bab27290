#!/usr/bin/env python3
"""mhw_composite()'s device pass on the resident float32 series of tools/bench_class_days.py: one JSON line.

    python tools/bench_composite.py [--cells 1036800] [--years 40] [--reps 10] [--blocks 256,512,4096,0] [--out FILE]

The series is generated on the device (the generator of bench.py) and the anchors are the event starts of the device
detect() stage on that series, the synthetic event table of tools/bench_objects.py and tools/bench_cooccurrence.py,
rasterised by xmhw_event_table_bits from rows with start == end.  Timed with HIP events around ONE C ABI call each, median
of --reps after a warm-up call, everything already on the device (the call looks up its two host tables in the
content-keyed cache first, as every stage entry does: that host time is inside the interval):
  * xmhw_composite_accumulate_f32 with before = after = 30 and before = 63, after = 64, one class and the four seasons, a
    constant base (one row) and a 366-row base;
  * the before = after = 30 and the (63, 64) one-class legs with every forced block length of --blocks (the integers must
    not change);
  * xmhw_class_sums_accumulate_f32 by year on the same series in the same run: the yardstick, a pass that reads every
    sample.
Reported with each leg: the ratio to the class-sums call and to the byte floor of what the design must move at 6.3 TB/s,
the measured copy rate -- the bitmap once, the rows of samples (and base rows) of the wave-steps on which some lane of the
wave has a window bit set, and the accumulator entries that are touched, 20 bytes each.  The share of wave-steps and of
lane-steps with a non-zero window is counted on the host from the bitmap of the first --count-cells cells."""
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


def window_shares(words, T, before, after):
    """(share of wave-steps, share of lane-steps) with a non-zero window, from bitmap words (W, n), n a multiple of 64"""
    W, n = words.shape
    bits = np.unpackbits(words.view(np.uint8).reshape(W, n, 8), axis=2, bitorder="little")       # (W, n, 64)
    A = bits.transpose(0, 2, 1).reshape(W * 64, n)[:T].astype(np.int32)                           # (T, n)
    # a window at step t holds the anchors of [t - after, t + before]
    csum = np.concatenate([np.zeros((1, n), np.int32), np.cumsum(A, axis=0, dtype=np.int32)])
    t = np.arange(T)
    lane = (csum[np.minimum(t + before, T - 1) + 1] - csum[np.maximum(t - after, 0)]) > 0
    wave = lane.reshape(T, n // 64, 64).any(axis=2)
    return float(wave.mean()), float(lane.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1036800)
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", default="256,512,4096,0")
    ap.add_argument("--count-cells", type=int, default=16384)
    ap.add_argument("--blocks-only", action="store_true", help="the forced block lengths alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_composite, hip_stress, require_gpu
    from xmhw_amd.calendar import add_doy
    from xmhw_amd.days_by import class_labels
    from xmhw_amd.detect_front import _check_inputs
    require_gpu()
    h, hc, hs = hip(), hip_composite(), hip_stress()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    T, C = t.shape[0], a.cells
    W = (T + 63) // 64
    year = class_labels("year", t)
    years = (year - year[0]).astype(np.int32)
    classes = {"all": (np.zeros(T, np.int32), 1), "season": (class_labels("season", t).astype(np.int32), 4)}
    res = {"bench": "composite", "T": int(T), "cells": C, "dtype": "float32", "hbm_bytes_per_s": HBM, "reps": a.reps}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    d_ts = dev.DeviceBuffer(4 * T * C)
    h.synth_sst(d_ts.ptr, 4, T, C, C, 0, 7, 0.0)
    h.stream_sync(0)
    d_cnt = dev.DeviceBuffer(8)

    # the anchors: the event starts of the device detect() stage on the same series
    doy = add_doy(t)
    plan = dev.Plan(doy, 5)
    Dc = plan.D
    _, _, _, crow = _check_inputs(np.zeros((T, 1), np.float32), np.zeros((Dc, 1)), np.zeros((Dc, 1)), doy, np.unique(doy))
    d_bits = dev.DeviceBuffer(8 * W * C)
    with dev.DeviceScope() as s:
        d_th, d_se, d_ex, d_n = s.alloc(8 * Dc * C), s.alloc(8 * Dc * C), s.alloc(8 * W * C), s.alloc(4 * C)
        d_off = s.alloc(8 * (C + 1))
        dev.clim_raw(plan, d_ts, 4, C, 0.9, False, d_th, d_se)
        h.exceed_bits(d_ts.ptr, 4, T, C, C, d_th.ptr, C, Dc, crow, 0, d_ex.ptr, C)
        h.events_from_bits(d_ex.ptr, T, C, C, 5, 1, 2, 0, d_n.ptr, 0)
        h.offsets_from_counts(d_n.ptr, C, d_off.ptr)
        h.stream_sync(0)
        n_events = int(d_off.to_array((C + 1,), np.int64)[-1])
        ncol = h.EVENT_COLUMNS
        d_tab = s.alloc(8 * max(n_events, 1) * ncol)
        h.events_from_bits(d_ex.ptr, T, C, C, 5, 1, 2, d_off.ptr, 0, d_tab.ptr)
        h.stream_sync(0)
        start = np.empty(max(n_events, 1), np.int32)
        step = 1 << 20
        chunk = np.empty((step, ncol), dtype=np.float64)
        for r0 in range(0, n_events, step):
            m = min(step, n_events - r0)
            h.memcpy_d2h(chunk[:m], d_tab.ptr + 8 * ncol * r0)
            start[r0:r0 + m] = chunk[:m, 0]           # the label of a row: its first step
        d_start, d_cell = s.upload(start), s.upload(np.arange(C, dtype=np.int64))
        h.event_table_bits(d_start.ptr, d_start.ptr, d_off.ptr, d_cell.ptr, C, T, d_bits.ptr, C)
        h.stream_sync(0)
    plan.destroy()
    res["events"] = n_events
    res["events_per_cell"] = round(n_events / C, 2)
    nc = min(C, a.count_cells) // 64 * 64
    words = np.empty((W, nc), np.uint64)
    for w in range(W):
        h.memcpy_d2h(words[w], d_bits.ptr + 8 * w * C)
    assert int(np.unpackbits(words.view(np.uint8)).sum()) > 0
    windows = ((30, 30), (63, 64))
    shares = {w: window_shares(words, T, *w) for w in windows}
    res["window_shares"] = [{"before": b, "after": f, "cells_counted": nc, "wave_steps_active": round(shares[(b, f)][0], 4),
                             "wave_steps_skipped": round(1.0 - shares[(b, f)][0], 4), "lane_steps_active": round(shares[(b, f)][1], 4)}
                            for b, f in windows]
    print(res["events_per_cell"], res["window_shares"], file=sys.stderr, flush=True)
    del words

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

    def leg(window, cname, Dr, block=0, keep=False):
        before, after = window
        D = before + after + 1
        kid, K = classes[cname]
        bufs = {"n": dev.DeviceBuffer(4 * K * D * C), "s": dev.DeviceBuffer(8 * K * D * C), "ss": dev.DeviceBuffer(8 * K * D * C)}
        ptrs = [bufs[k].ptr for k in ("n", "s", "ss")]
        hc.set_composite_block(block)
        hc.composite_init(K, D, C, *ptrs, C, d_cnt.ptr)
        call = lambda: hc.composite_accumulate(d_ts.ptr, 4, T, C, C, bases[Dr].ptr, C, Dr, rows[Dr], 0, d_bits.ptr, C, kid, K,  # noqa: E731
                                               before, after, *ptrs, C, d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        hc.composite_init(K, D, C, *ptrs, C, d_cnt.ptr)
        call()
        h.stream_sync(0)
        n = bufs["n"].to_array((K, D, C), np.int32)
        out = (n, bufs["s"].to_array((K, D, C), np.int64), bufs["ss"].to_array((K, D, C), np.int64)) if keep else None
        n_range = int(d_cnt.to_array((1,), np.int64)[0])
        for b in bufs.values():
            b.free()
        pairs, touched = int(n.astype(np.int64).sum()), int(np.count_nonzero(n))
        wave_share = shares[window][0]
        floor = (8 * W * C + wave_share * T * C * (4 + (8 if Dr > 1 else 0)) + 20 * touched) / HBM * 1e3
        return {"before": before, "after": after, "D": D, "classes": cname, "K": K, "base_rows": Dr, "block": block,
                "ms": round(ms, 3), "ms_all": every, "byte_floor_ms": round(floor, 3), "over_floor": round(ms / floor, 2),
                "over_class_sums": round(ms / yard, 2), "pairs": pairs, "pairs_per_s": round(pairs / (ms * 1e-3), -8),
                "entries_touched": touched, "n_range": n_range}, out

    res["legs"] = []
    for Dr in (1, 366) if not a.blocks_only else ():
        if Dr == 366:
            bases[366] = dev.DeviceBuffer.from_array(np.full((366, C), 15.0) + 0.01 * np.arange(366)[:, None])
        for cname in ("all", "season"):
            for window in windows:
                r, _ = leg(window, cname, Dr)
                assert r["n_range"] == 0 and r["pairs"] > 0, r
                res["legs"].append(r)
                print(r, file=sys.stderr, flush=True)
                dump()
    if bases[366] is not None:
        bases[366].free()

    # forced block lengths: same integers
    res["forced_blocks"] = []
    for window in windows:
        ref = None
        for block in [int(b) for b in a.blocks.split(",")] + [T]:
            r, out = leg(window, "all", 1, block=block, keep=True)
            ref = out if ref is None else ref
            r["identical_integers"] = bool(all(np.array_equal(x, y) for x, y in zip(out, ref)))
            assert r["identical_integers"], f"block {block} changed the result"
            res["forced_blocks"].append(r)
            print(r, file=sys.stderr, flush=True)
        del ref, out
    hc.set_composite_block(0)
    for b in (d_ts, d_cnt, d_bits, bases[1]):
        b.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
