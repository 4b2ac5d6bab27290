#!/usr/bin/env python3
"""mhw_rank() on a synthetic event table shaped like a 0.25-degree detect() result: one JSON line.

    python tools/bench_rank.py [--cells 259200] [--mean 60] [--big 4] [--big-size 5000] [--reps 5]

Cells get Poisson(mean) events (a few get big-size), 31 float64 columns: continuous ones, integer-valued
durations and category, some NaN.  Reported: the device time of the rank launches alone (HIP events
around xmhw_event_rank; median of reps, table already on the device), the wall time of a whole
mhw_rank() call (upload, kernels, download, the two EventDataset), the bytes the kernels must move
(every table row read once, the 24 ranks and 24 return periods written) and the time those bytes take
at 6.3 TB/s (HBM, measured copy rate)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12


def synth(cells, mean, big, big_size, seed=1):
    from xmhw_amd.detect import EventDataset
    rng = np.random.default_rng(seed)
    sizes = rng.poisson(mean, cells).astype(np.int64)
    sizes[rng.choice(cells, big, replace=False)] = big_size
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offsets[-1])
    cols = EventDataset.columns
    tab = rng.standard_normal((n, len(cols)))
    for name in ("duration", "duration_moderate", "duration_strong", "duration_severe", "duration_extreme"):
        tab[:, cols.index(name)] = rng.integers(0, 40, n)
    tab[:, cols.index("category")] = rng.integers(1, 5, n)
    tab[rng.random(n) < 0.01, cols.index("rate_onset")] = np.nan
    tab[:, 0] = np.concatenate([np.arange(s) for s in sizes])
    return tab, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=259200)
    ap.add_argument("--mean", type=float, default=60.0)
    ap.add_argument("--big", type=int, default=4)
    ap.add_argument("--big-size", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.detect import EventDataset
    from xmhw_amd.device import DeviceBuffer
    from xmhw_amd.rank import RANKED, mhw_rank
    require_gpu()
    h = hip()
    tab, off = synth(a.cells, a.mean, a.big, a.big_size)
    n, C = tab.shape[0], off.shape[0] - 1
    cols = [EventDataset.columns.index(k) for k in RANKED]
    ld_out = 1 + len(cols)
    d_tab, d_off = DeviceBuffer.from_array(tab), DeviceBuffer.from_array(off)
    d_r, d_p = DeviceBuffer(8 * n * ld_out), DeviceBuffer(8 * n * ld_out)
    e0, e1 = h.event_create(), h.event_create()
    ms = []
    for _ in range(a.reps + 1):
        h.event_record(e0, 0)
        h.event_rank(d_tab.ptr, tab.shape[1], d_off.ptr, C, cols, 40.0, d_r.ptr + 8, d_p.ptr + 8, ld_out)
        h.event_record(e1, 0)
        h.stream_sync(0)
        ms.append(h.event_elapsed_ms(e0, e1))
    # spot check: a few cells against the stable-argsort definition
    r = d_r.to_array((n, ld_out), np.float64)
    rng = np.random.default_rng(2)
    checked = [int(c) for c in rng.choice(C, 64, replace=False)] + [int(np.argmax(np.diff(off)))]
    for c in checked:
        for k, col in enumerate(cols):
            v = tab[off[c]:off[c + 1], col]
            ok = ~np.isnan(v)
            want = np.full(v.shape, np.nan)
            want[ok] = ok.sum() - np.argsort(np.argsort(v[ok], kind="stable"), kind="stable")
            np.testing.assert_array_equal(r[off[c]:off[c + 1], 1 + k], want)
    for b in (d_tab, d_off, d_r, d_p):
        b.free()
    h.event_destroy(e0)
    h.event_destroy(e1)
    mhw = EventDataset(tab, off, np.datetime64("1982-01-01") + np.arange(14610), np.arange(C), np.ones(C, bool),
                       ("cell",), (C,), {"cell": np.arange(C)}, {}, {}, {}, False)
    t0 = time.perf_counter()
    mhw_rank(mhw)
    wall = time.perf_counter() - t0
    read = 8 * n * tab.shape[1] + 8 * (C + 1)
    written = 2 * 8 * n * len(cols)
    kernel = float(np.median(ms[1:]))
    print(json.dumps({"bench": "mhw_rank", "cells": C, "events": n, "max_cell": int(np.diff(off).max()),
                      "columns": len(cols), "kernel_ms": round(kernel, 3), "kernel_ms_all": [round(x, 3) for x in ms[1:]],
                      "mhw_rank_s": round(wall, 3), "bytes_read": read, "bytes_written": written,
                      "hbm_floor_ms": round((read + written) / HBM * 1e3, 3),
                      "x_floor": round(kernel / ((read + written) / HBM * 1e3), 2), "cells_checked": len(checked)}))


if __name__ == "__main__":
    main()
