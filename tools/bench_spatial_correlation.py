#!/usr/bin/env python3
"""spatial_correlation()'s device pass on the resident float32 series of tools/bench_lag_correlation.py, taken as an
uncompacted ny x 1440 grid: one JSON line.

    python tools/bench_spatial_correlation.py [--ny 720] [--nx 1440] [--years 40] [--reps 5] [--blocks 256,4096,0]
                                              [--out FILE]

The series is generated on the device (the generator of bench.py: the points are independent, which changes no
instruction of the pass).  Timed with HIP events around ONE C ABI call each, median of --reps after a warm-up call,
everything already on the device (the call looks up its three host tables in the content-keyed cache first, as every stage
entry does: that host time is inside the interval):
  * xmhw_spatial_corr_accumulate_f32 with D = 1 / 8 / 13 (what the device sees of the default cross, reach (8, 8)) / 16 /
    64 offsets of the half-plane; one class and the four seasons; a constant base (one row) and a 366-row base;
  * D = 8 and 64 by season on a series with 5 % scattered NaN;
  * D = 13 and 64 of one class with every forced block length of --blocks (the integers must not change): what the
    automatic rule of csrc/stage_blocks.h rests on;
  * D = 13 and 64 of one class under both tile shapes, 4 x 64 and 8 x 64 (the integers must not change);
  * the comparator, in the same run on the same series: xmhw_lag_corr_accumulate_f32 (autocorrelation) with as many lags
    as there are offsets.  It forms the same six sums per pair, so its pairs per second are the yardstick.
Reported with each leg: the ratio to the byte floor at 6.3 TB/s -- every sample and base row once and the 44 bytes of
every accumulator entry that is touched --, the valid pairs per second and their ratio to the comparator's."""
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


def bench_offsets(D):
    """D offsets of the half-plane, (0, 0) first: the default cross, then the cross of reach (32, 32), then near diagonals"""
    from xmhw_amd.spatial_correlation import cross_offsets, half_plane
    near = [tuple(v) for v in half_plane(cross_offsets((8, 8)))[0].tolist()]
    far = [tuple(v) for v in half_plane(cross_offsets((32, 32)))[0].tolist()]
    diag = [(dj, di) for dj in range(1, 9) for di in (-4, -3, -2, -1, 1, 2, 3, 4)]
    pool = list(dict.fromkeys(near + (diag if D <= 16 else far + diag)))
    if D == 8:
        pool = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (2, 0), (3, 0)]
    return np.array(pool[:D], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=720)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", default="256,4096,0")
    ap.add_argument("--short", action="store_true", help="one class and a constant base alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_lagcorr, hip_spatialcorr, require_gpu
    from xmhw_amd.days_by import class_labels
    require_gpu()
    h, hl, hs = hip(), hip_lagcorr(), hip_spatialcorr()
    t = np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]")
    T, ny, nx = t.shape[0], a.ny, a.nx
    N = ny * nx
    classes = {"all": (np.zeros(T, np.int32), 1), "season": (class_labels("season", t).astype(np.int32), 4)}
    res = {"bench": "spatial_correlation", "T": int(T), "ny": ny, "nx": nx, "points": N, "dtype": "float32",
           "hbm_bytes_per_s": HBM, "reps": a.reps}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    def series(seed, nan_frac=0.0):
        d = dev.DeviceBuffer(4 * T * N)
        h.synth_sst(d.ptr, 4, T, N, N, 0, seed, nan_frac)
        h.stream_sync(0)
        return d

    d_x = series(7)
    d_cnt = dev.DeviceBuffer(16)
    bases = {1: dev.DeviceBuffer.from_array(np.full((1, N), 15.0)), 366: None}
    rows = {1: np.zeros(T, np.int32), 366: (np.arange(T) % 366).astype(np.int32)}

    def finish(r, n, ms, every, Dr):
        pairs, touched = int(n.astype(np.int64).sum()), int(np.count_nonzero(n))
        floor = (T * N * (4 + (8 if Dr > 1 else 0)) + 44 * touched) / HBM * 1e3
        r.update(ms=round(ms, 3), ms_all=every, byte_floor_ms=round(floor, 3), over_floor=round(ms / floor, 2), pairs=pairs,
                 pairs_per_s=round(pairs / (ms * 1e-3), -8), entries_touched=touched)
        return r

    def leg(d_a, D, cname, Dr, block=0, tile=0, keep=False, what="spatial"):
        kid, K = classes[cname]
        off = bench_offsets(D)
        bufs = {k: dev.DeviceBuffer((4 if k == "n" else 8) * K * D * N) for k in FIELDS}
        ptrs = [bufs[k].ptr for k in FIELDS]
        hs.set_spatial_corr_block(block)
        hs.set_spatial_corr_tile(tile)
        hs.spatial_corr_init(K, D, ny, nx, *ptrs, N, d_cnt.ptr)
        call = lambda: hs.spatial_corr_accumulate(d_a.ptr, 4, N, 0, T, T, ny, nx, 1, bases[Dr].ptr, N, Dr, rows[Dr], 0, kid, K,  # noqa: E731
                                                  off, *ptrs, N, d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        hs.spatial_corr_init(K, D, ny, nx, *ptrs, N, d_cnt.ptr)
        call()
        h.stream_sync(0)
        n = bufs["n"].to_array((K, D, N), np.int32)
        # (at 64 offsets the comparison reads back n and sxy alone: 1.6 of 2.9 GB less per setting)
        out = tuple([n] + [bufs[k].to_array((K, D, N), np.int64) for k in (FIELDS[1:] if D <= 16 else ("sxy",))]) if keep else None
        n_range = int(d_cnt.to_array((1,), np.int64)[0])
        for b in bufs.values():
            b.free()
        r = finish({"what": what, "offsets": D, "classes": cname, "K": K, "base_rows": Dr, "block": block, "tile_rows": tile or 8,
                    "n_range": n_range}, n, ms, every, Dr)
        return r, out

    def lag_leg(d_a, nlags, cname, Dr):
        """the comparator: the autocorrelation with ``nlags`` lags on the same series, every grid point a cell"""
        kid, K = classes[cname]
        bufs = {k: dev.DeviceBuffer((4 if k == "n" else 8) * K * nlags * N) for k in FIELDS}
        ptrs = [bufs[k].ptr for k in FIELDS]
        hl.set_lag_corr_block(0)
        hl.lag_corr_init(K, nlags - 1, N, *ptrs, N, d_cnt.ptr)
        call = lambda: hl.lag_corr_accumulate(d_a.ptr, N, d_a.ptr, N, 4, T, N, bases[Dr].ptr, N, bases[Dr].ptr, N, Dr, rows[Dr],  # noqa: E731
                                              0, 0, kid, K, nlags - 1, *ptrs, N, d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        hl.lag_corr_init(K, nlags - 1, N, *ptrs, N, d_cnt.ptr)
        call()
        h.stream_sync(0)
        n = bufs["n"].to_array((K, nlags, N), np.int32)
        for b in bufs.values():
            b.free()
        return finish({"what": "lag_correlation, the comparator", "lags": nlags, "classes": cname, "K": K, "base_rows": Dr},
                      n, ms, every, Dr)

    res["legs"], res["comparator"] = [], []
    yard = {}

    def record(r, where="legs"):
        res[where].append(r)
        print(r, file=sys.stderr, flush=True)
        dump()

    for Dr in (1,) if a.short else (1, 366):
        if Dr == 366:
            bases[366] = dev.DeviceBuffer.from_array(np.full((366, N), 15.0) + 0.01 * np.arange(366)[:, None])
        for cname in ("all",) if a.short else ("all", "season"):
            for D in (1, 8, 13, 16, 64):
                c = lag_leg(d_x, D, cname, Dr)
                record(c, "comparator")
                yard[(D, cname, Dr)] = c["pairs_per_s"]
                r, _ = leg(d_x, D, cname, Dr)
                assert r["n_range"] == 0 and r["pairs"] > 0, r
                r["pairs_per_s_over_lag_corr"] = round(r["pairs_per_s"] / c["pairs_per_s"], 3)
                record(r)
    if bases[366] is not None:
        bases[366].free()
    if not a.short:
        d_gaps = series(7, 0.05)
        for D in (8, 64):
            r, _ = leg(d_gaps, D, "season", 1, what="spatial, 5 % scattered NaN")
            record(r)
        d_gaps.free()

    # forced block lengths and both tile shapes: same integers
    res["forced_blocks"], res["tile_shapes"] = [], []
    for D in (13, 64):
        ref = None
        for where, settings in (("forced_blocks", [(int(b), 0) for b in a.blocks.split(",")] + [(T, 0)]),
                                ("tile_shapes", [(0, 4), (0, 8)])):
            for block, tile in settings:
                r, out = leg(d_x, D, "all", 1, block=block, tile=tile, keep=True)
                ref = out if ref is None else ref
                r["identical_integers"] = bool(all(np.array_equal(u, v) for u, v in zip(out, ref)))
                assert r["identical_integers"], f"block {block}, tile {tile} changed the result"
                r["pairs_per_s_over_lag_corr"] = round(r["pairs_per_s"] / yard[(D, "all", 1)], 3)
                record(r, where)
        del ref, out
    hs.set_spatial_corr_block(0)
    hs.set_spatial_corr_tile(0)
    for b in (d_x, d_cnt, bases[1]):
        b.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
