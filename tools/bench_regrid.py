#!/usr/bin/env python3
"""regrid()'s device pass on the resident float32 series of tools/bench_coarsen.py, an uncompacted ny x 1440 grid of
0.25 degree cells (ny = 720: the globe; ny = 360: 45 S to 45 N, the half grid): one JSON line.

    python tools/bench_regrid.py [--ny 720] [--years 40] [--reps 3] [--out FILE]

The series is generated on the device (the generator of bench.py).  Timed with HIP events around ONE C ABI call each,
median of --reps after a warm-up call, everything already on the device (the call looks up its overlap tables in the
content-keyed cache first, as every stage entry does: that host time is inside the interval).  The tables are those of
xmhw_amd.regrid.overlap_table() on real grids, latitude weighed on the sphere.  The legs, each on the direct path
(variant 1), on the staged path (variant 2) and as the automatic choice takes it (the bits of the first and the last
steps must not differ):
  * 0.25 -> 1 degree, aligned (4 x 4 footprints)
  * 0.25 -> an ERA5-style 0.25 degree grid shifted by half a cell, latitude descending (2 x 2 footprints)
  * 1 -> 0.25 degree (1 x 1 footprints, every source sample feeds 16 cells), on a 1 degree series of its own, the output
    as large as the 0.25 degree series
  * 0.25 -> 2.5 degree (10 x 10 footprints)
The comparator, in the same run on the same series: xmhw_coarsen_f32 at (4, 4, 1) with wi[j, i] = ay[j] * 4096, whose
bits the aligned 0.25 -> 1 degree leg must reproduce exactly.  Reported with each leg: the ratio to the byte floor at
6.3 TB/s -- every input sample once and every output entry once -- and the ratio to the comparator."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
PATHS = ("none", "direct", "staged")


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
    ap.add_argument("--years", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import xmhw_amd.device as dev
    from xmhw_amd._lib import hip, hip_coarsen, hip_regrid, require_gpu
    from xmhw_amd.regrid import axis_bounds, overlap_table
    require_gpu()
    h, hc, hr = hip(), hip_coarsen(), hip_regrid()
    T = int(np.arange("1982-01-01", f"{1982 + a.years}-01-01", dtype="datetime64[D]").shape[0])
    ny, nx = a.ny, 1440
    if ny % 20:
        raise SystemExit("--ny should be a multiple of 20 (whole 2.5 degree and 1 degree cells)")
    edge = ny * 0.125                                             # the grid covers latitudes -edge .. edge
    res = {"bench": "regrid", "T": T, "ny": ny, "nx": nx, "points": ny * nx, "hbm_bytes_per_s": HBM, "reps": a.reps}

    def dump():
        if a.out:
            with open(a.out, "w") as fo:
                fo.write(json.dumps(res) + "\n")

    def record(r, where="legs"):
        res.setdefault(where, []).append(r)
        print(r, file=sys.stderr, flush=True)
        dump()

    def series(seed, n, steps=T):
        d = dev.DeviceBuffer(4 * steps * n)
        h.synth_sst(d.ptr, 4, steps, n, n, 0, seed, 0.0)
        h.stream_sync(0)
        return d

    def grid(step, descending=False, shifted=False):
        """(lat bounds, lon bounds) of a grid of `step` degrees over the same latitudes; shifted: centres on the bounds
        of the unshifted grid (the first and the last row are half cells), longitude from -step / 2"""
        if shifted:
            lat = axis_bounds(np.arange(-edge, edge + step / 2, step), (-edge, edge))
            lon = np.arange(-step / 2, 360.0, step)
        else:
            lat, lon = np.arange(-edge, edge + step / 2, step), np.arange(0.0, 360.0 + step / 2, step)
        return (lat[::-1].copy() if descending else lat), lon

    def tables(src, dst):
        rows = overlap_table(src[0], dst[0], "sphere")
        cols = overlap_table(src[1], dst[1], "plane", 360.0)
        return rows, cols

    d_cnt = dev.DeviceBuffer.from_array(np.zeros(1, np.int64))
    KEEP = 4                                                     # the first and the last steps compared

    def leg(d_x, sny, snx, rows, cols, variant, what):
        my, mx = len(rows[0]), len(cols[0])
        cells = my * mx
        d_out = dev.DeviceBuffer(4 * T * cells)
        hr.set_regrid_variant(variant)
        path = hr.regrid_class(snx, rows[1], cols[0], cols[1], 1)
        call = lambda: hr.regrid(d_x.ptr, 4, T, sny * snx, sny, snx, *rows, *cols, 1, 15.0, 32768, d_out.ptr, cells,  # noqa: E731
                                 0, 0, d_cnt.ptr)
        ms, every = median_ms(h, call, a.reps)
        out = np.empty((2, KEEP, cells), np.float32)
        h.memcpy_d2h(out[0], d_out.ptr)
        h.memcpy_d2h(out[1], d_out.ptr + 4 * (T - KEEP) * cells)
        d_out.free()
        hr.set_regrid_variant(0)
        read, written = 4 * T * sny * snx, 4 * T * cells
        floor = (read + written) / HBM * 1e3
        return {"what": what, "source": [sny, snx], "destination": [my, mx],
                "footprint": [int(np.diff(rows[1]).max()), int(np.diff(cols[1]).max())], "variant": variant, "path": PATHS[path],
                "ms": round(ms, 3), "ms_all": every, "bytes_read": read, "bytes_written": written,
                "byte_floor_ms": round(floor, 3), "over_floor": round(ms / floor, 2)}, out

    quarter, one = grid(0.25), grid(1.0)
    d_x = series(7, ny * nx)
    # the comparator: coarsen() at (4, 4, 1) under the weights of the aligned leg
    rows1, cols1 = tables(quarter, one)
    assert (cols1[2] == 4096).all() and (np.diff(rows1[1]) == 4).all() and (rows1[0] == 4 * np.arange(ny // 4)).all()
    wi = np.repeat(rows1[2].astype(np.int64) * 4096, nx).astype(np.int32)
    d_wi = dev.DeviceBuffer.from_array(wi)
    cells1 = (ny // 4) * (nx // 4)
    d_c = dev.DeviceBuffer(4 * T * cells1)
    win = np.arange(T + 1, dtype=np.int32)
    ms, every = median_ms(h, lambda: hc.coarsen(d_x.ptr, 4, T, ny * nx, ny, nx, 4, 4, ny // 4, nx // 4, d_wi.ptr, 15.0, 32768,
                                                win, d_c.ptr, cells1, 0, 0, d_cnt.ptr), a.reps)
    ref = np.empty((2, KEEP, cells1), np.float32)
    h.memcpy_d2h(ref[0], d_c.ptr)
    h.memcpy_d2h(ref[1], d_c.ptr + 4 * (T - KEEP) * cells1)
    floor = (4 * T * ny * nx + 4 * ny * nx + 4 * T * cells1) / HBM * 1e3
    comparator = {"what": "xmhw_coarsen_f32 at (4, 4, 1): the comparator", "ms": round(ms, 3), "ms_all": every,
                  "byte_floor_ms": round(floor, 3), "over_floor": round(ms / floor, 2)}
    record(comparator, "comparator")
    for b in (d_wi, d_c):
        b.free()

    def run(d_src, sny, snx, rows, cols, what, want=None):
        first = None
        for variant in (1, 2, 0):
            r, out = leg(d_src, sny, snx, rows, cols, variant, what)
            first = out if first is None else first
            r["identical_bits"] = bool(np.array_equal(out.view(np.uint32), first.view(np.uint32)))
            assert r["identical_bits"], f"variant {variant} changed the result"
            if want is not None:
                same = np.isnan(out) == np.isnan(want)
                r["equals_coarsen"] = bool(same.all() and np.array_equal(out[~np.isnan(out)].view(np.uint32),
                                                                         want[~np.isnan(want)].view(np.uint32)))
                assert r["equals_coarsen"], "the aligned leg differs from coarsen()"
            r["over_comparator"] = round(r["ms"] / comparator["ms"], 3)
            record(r)

    run(d_x, ny, nx, rows1, cols1, "0.25 -> 1 degree, aligned", want=ref)
    run(d_x, ny, nx, *tables(quarter, grid(0.25, descending=True, shifted=True)), "0.25 -> ERA5-style 0.25 degree, shifted, descending")
    run(d_x, ny, nx, *tables(quarter, grid(2.5)), "0.25 -> 2.5 degree")
    d_x.free()
    d_one = series(9, (ny // 4) * (nx // 4))
    run(d_one, ny // 4, nx // 4, *tables(one, quarter), "1 -> 0.25 degree")
    d_one.free()
    assert int(d_cnt.to_array((1,), np.int64)[0]) == 0, "samples out of range"
    d_cnt.free()
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
