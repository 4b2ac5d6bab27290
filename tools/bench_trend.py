#!/usr/bin/env python3
"""mean_trend() on synthetic planes shaped like the block_average() result of a 0.25-degree grid: one JSON line.

    python tools/bench_trend.py [--stats 22] [--blocks 40] [--cols 1036800] [--reps 5] [--sample 4096]

A third of the columns are all-NaN (land); every other statistic is integer-valued (counts: ties), the rest
continuous; 2 % of the ocean blocks are NaN.  Reported: the device time of each kernel (HIP events around the C ABI
call, median of reps, planes already on the device), the wall time of a whole mean_trend() call per method
(upload, kernel, download, the host's mk_z / p_value), the bytes each kernel must move (every plane value read
once, the output planes written) and the time those bytes take at 6.3 TB/s (HBM, measured copy rate), the work the
Theil-Sen design implies per ocean item, and the CPU route this replaces: the numpy oracle of the tests on a sample
of columns (and scipy.stats.theilslopes per series where scipy is installed), as time per item."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 6.3e12


def synth(nstat, nb, C, seed=1):
    rng = np.random.default_rng(seed)
    p = np.empty((nstat, nb, C))
    for s in range(nstat):
        if s % 2 == 0:
            p[s] = rng.poisson(2.0 + s, (nb, C))
        else:
            p[s] = rng.standard_normal((nb, C)) + 0.02 * np.arange(nb)[:, None]
        p[s][rng.random((nb, C)) < 0.02] = np.nan
    land = rng.random(C) < 1 / 3
    p[:, :, land] = np.nan
    return p, land


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stats", type=int, default=22)
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--cols", type=int, default=1036800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=4096)
    a = ap.parse_args()
    import trend_oracle as to
    from xmhw_amd import BlockDataset, mean_trend
    from xmhw_amd import trend as tr
    from xmhw_amd._lib import hip, require_gpu
    from xmhw_amd.device import DeviceBuffer
    require_gpu()
    h = hip()
    nstat, nb, C = a.stats, a.blocks, a.cols
    p, land = synth(nstat, nb, C)
    print("planes ready", file=sys.stderr, flush=True)
    x = tr.centred_years(1982.0 + np.arange(nb))
    tc = tr.tcrit_table(0.05, nb)
    d_in, d_x, d_t = DeviceBuffer.from_array(p), DeviceBuffer.from_array(x), DeviceBuffer.from_array(tc)
    d_out = DeviceBuffer(8 * 4 * nstat * C)
    e0, e1 = h.event_create(), h.event_create()
    ms = {"ols": [], "theil_sen": []}
    got = {}
    for method in ms:
        for _ in range(a.reps + 1):
            h.event_record(e0, 0)
            if method == "ols":
                h.block_trend_ols(d_in.ptr, nstat, nb, C, C, d_x.ptr, d_t.ptr, d_out.ptr, C)
            else:
                h.block_trend_theil_sen(d_in.ptr, nstat, nb, C, C, d_x.ptr, d_out.ptr, C)
            h.event_record(e1, 0)
            h.stream_sync(0)
            ms[method].append(h.event_elapsed_ms(e0, e1))
        nwhat = 3 if method == "ols" else 4
        got[method] = d_out.to_array((4, nstat, C), np.float64)[:nwhat]
    for b in (d_in, d_x, d_t, d_out):
        b.free()
    h.event_destroy(e0)
    h.event_destroy(e1)
    print("kernels timed", {k: v[1:] for k, v in ms.items()}, file=sys.stderr, flush=True)
    # the CPU route on a sample of columns, which is also the spot check (bit for bit)
    rng = np.random.default_rng(2)
    sample = np.sort(rng.choice(C, min(a.sample, C), replace=False))
    cpu = {}
    for method in ms:
        t0 = time.perf_counter()
        want = to.trend_oracle(p[:, :, sample], x, tc, method)
        cpu[method] = time.perf_counter() - t0
        g = got[method][:, :, sample]
        assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(g[~np.isnan(want)], want[~np.isnan(want)]), method
    n_sample = nstat * sample.size
    scipy_us = None
    try:
        from scipy.stats import theilslopes
        cols = sample[~land[sample]][:64]
        t0 = time.perf_counter()
        for c in cols:
            for s in range(nstat):
                y = p[s, :, c]
                v = ~np.isnan(y)
                theilslopes(y[v], x[v])
        scipy_us = (time.perf_counter() - t0) / (len(cols) * nstat) * 1e6
    except ImportError:
        pass
    names = [f"stat{s:02d}" for s in range(nstat)]
    blk = BlockDataset({k: p[s] for s, k in enumerate(names)}, ("years", "cell"),
                       {"years": 1982 + np.arange(nb), "cell": np.arange(C)}, 1982 + np.arange(nb + 1))
    wall = {}
    for method in ms:
        t0 = time.perf_counter()
        mean_trend(blk, method=method)
        wall[method] = time.perf_counter() - t0
        print("mean_trend", method, wall[method], file=sys.stderr, flush=True)
    items = nstat * C
    ocean_items = nstat * int((~land).sum())
    m_mean = float((~np.isnan(p[:, :, ~land])).sum(axis=1).mean()) if ocean_items else 0.0
    pairs = nb * (nb - 1) // 2
    read = 8 * nstat * nb * C
    out = {"bench": "mean_trend", "stats": nstat, "blocks": nb, "cols": C, "items": items, "ocean_items": ocean_items,
           "mean_valid_blocks": round(m_mean, 2), "bytes_read": read}
    for method, nwhat in (("ols", 3), ("theil_sen", 4)):
        k = float(np.median(ms[method][1:]))
        floor = (read + 8 * nwhat * items) / HBM * 1e3
        out[method] = {"kernel_ms": round(k, 3), "kernel_ms_all": [round(v, 3) for v in ms[method][1:]],
                       "bytes_written": 8 * nwhat * items, "hbm_floor_ms": round(floor, 3), "x_floor": round(k / floor, 2),
                       "mean_trend_s": round(wall[method], 3),
                       "gpu_ns_per_item": round(k * 1e6 / items, 3),
                       "cpu_oracle_us_per_item": round(cpu[method] / n_sample * 1e6, 3),
                       "cpu_oracle_over_gpu_kernel": round(cpu[method] / n_sample / (k * 1e-3 / items), 1)}
    # per ocean item with all nb blocks valid: one division per pair; the radix select reads every stored key once
    # per pass (at most 8 passes of 8 bits, fewer when one candidate is left) plus one or two closing passes
    out["theil_sen"].update({"divisions_per_full_item": pairs, "select_key_reads_per_full_item_max": pairs * 10,
                             "rank_compares_per_full_item": nb * nb,
                             "scipy_theilslopes_us_per_item": None if scipy_us is None else round(scipy_us, 1),
                             "sample_columns_checked": int(sample.size)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
