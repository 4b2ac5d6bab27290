"""Cases and child-process worker of tests/test_gpu_sorted_onerow.py and tests/test_host_sorted_onerow.py: one-row chunks
(Feb 29 of a daily record) of the sorted-list kernel, settled directly or -- XMHW_SORTED_ONEROW=0, a process-wide switch
read once, hence the child processes -- by walking their table rows.

    python tests/sorted_onerow_cases.py ROOT gpu OUT.npz     every case on the GPU: sorted (and generic) thresh / seas
    python tests/sorted_onerow_cases.py ROOT host OUT.npz    the plan queries of every record, no GPU
"""
import os
import sys

import numpy as np

# (name, first day, day after the last): daily records, each with at least one Feb 29
RECORDS = [
    ("12y", "1981-01-01", "1993-01-01"),                    # 6 tracks per lane, 3 leap tracks
    ("16y_leap_start", "1980-01-01", "1996-01-01"),         # 8 tracks per lane (the three-wave build); starts in a leap year
    ("37y_feb29_start", "1984-02-29", "2021-01-01"),        # 19 tracks per lane, the last one padding; starts on Feb 29
    ("40y", "1982-01-01", "2022-01-01"),                    # the headline record: 10 leap tracks
    ("48y", "1976-01-01", "2024-01-01"),                    # 12 leap tracks: pools of 132 samples, the largest admitted
    ("40y_partial_last", "1982-01-01", "2021-03-15"),       # a partial last year
    ("9y_one_leap", "1897-01-01", "1906-01-01"),            # exactly one leap year (1900 is none)
]
# further record lengths the host test asks the plan about
HOST_YEARS = (12, 16, 37, 40, 43, 48)
CELLS = (1, 31, 33, 65)
QS = (0.85, 0.9, 0.99, 1.0, 0.15, 0.1, 0.0)
KINDS = ("noise", "quantised", "constant", "inf_zero", "nan5", "leap_all_nan", "leap_one_valid", "wide")


def doy_of(start, stop):
    import xmhw_oracle as ora
    return ora.add_doy(np.arange(start, stop, dtype="datetime64[D]"))


def cases():
    """(record index, C, q, negate): every record x every cell count, the quantiles and both signs dealt round, plus the
    largest pools at the two quantiles that reach deepest into them and the headline shape"""
    out = []
    idx = 0
    for r in range(len(RECORDS)):
        for C in CELLS:
            out.append((r, C, QS[idx % len(QS)], (idx // len(QS)) % 2 == 1))
            idx += 1
    out += [(4, 33, 0.85, False), (4, 31, 0.15, True), (4, 65, 0.15, False), (3, 65, 0.9, False), (3, 33, 0.1, True)]
    return out


def series(case_no, start, stop, C):
    """float32 (T, C + 7): the cells take the KINDS in turn (a one-cell grid: by case number); the 7 columns of pitch hold
    a value no cell has"""
    time = np.arange(start, stop, dtype="datetime64[D]")
    T = time.shape[0]
    rng = np.random.default_rng(1000 + case_no)
    t = np.arange(T)[:, None]
    x = (15.0 + rng.uniform(2, 10, C) * np.sin(2 * np.pi * (t - rng.uniform(0, 365, C)) / 365.25)
         + rng.normal(size=(T, C))).astype(np.float32)
    md = (time - time.astype("datetime64[Y]")).astype(int)                 # day of the year, 0-based
    leap = np.array([(y % 4 == 0 and y % 100 != 0) or y % 400 == 0 for y in time.astype("datetime64[Y]").astype(int) + 1970])
    feb29 = leap & (md == 59)
    pool = np.zeros(T, dtype=bool)                                         # the samples the Feb-29 row pools
    for i in np.flatnonzero(feb29):
        pool[max(i - 5, 0):i + 6] = True
    for c in range(C):
        kind = KINDS[(c + case_no) % len(KINDS)]
        if kind == "quantised":
            x[:, c] = np.round(x[:, c] / 0.01) * 0.01
        elif kind == "constant":
            x[:, c] = 17.25
        elif kind == "inf_zero":
            r = rng.random(T)
            x[r < 0.04, c] = np.inf
            x[(r >= 0.04) & (r < 0.08), c] = -np.inf
            x[(r >= 0.08) & (r < 0.5), c] = 0.0
            x[(r >= 0.5) & (r < 0.9), c] = -0.0
        elif kind == "nan5":
            x[rng.random(T) < 0.05, c] = np.nan
        elif kind == "leap_all_nan":
            x[pool, c] = np.nan
        elif kind == "leap_one_valid":
            keep = rng.choice(np.flatnonzero(pool))
            x[pool, c] = np.nan
            x[keep, c] = 3.5
        elif kind == "wide":
            # (positive, 60 decades apart: every float64 sum is inexact, so the order of the sums shows in `seas`)
            x[:, c] = (10.0 ** rng.uniform(-30, 30, T)).astype(np.float32)
    full = np.full((T, C + 7), 1.0e9, dtype=np.float32)
    full[:, :C] = x
    return full


def run_gpu(out_path):
    import xmhw_amd.device as dev
    from xmhw_amd._lib import require_gpu
    require_gpu()
    h = dev.hip()
    res = {}
    for no, (r, C, q, negate) in enumerate(cases()):
        _, start, stop = RECORDS[r]
        doy = doy_of(start, stop)
        x = series(no, start, stop, C)
        ld, ldo = C + 7, C + 3
        for kernel in ("auto", "generic"):
            plan = dev.Plan(doy, 5, kernel=kernel)
            bufs = [dev.DeviceBuffer.from_array(x)]
            try:
                if kernel == "auto":
                    res[f"layout_{no}"] = plan.layout_in_use()
                    res[f"direct_{no}"] = plan.sorted_direct(C)
                    res[f"row_{no}"] = int(np.searchsorted(plan.doys, 60))
                fill = np.full((plan.D, ldo), -7.0)
                bufs += [dev.DeviceBuffer.from_array(fill), dev.DeviceBuffer.from_array(fill)]
                dev.clim_raw(plan, bufs[0], 4, C, q, negate, bufs[1], bufs[2], ld=ld, ldo=ldo)
                h.stream_sync(0)
                th, se = (b.to_array((plan.D, ldo), np.float64) for b in bufs[1:])
                assert np.all(th[:, C:] == -7.0) and np.all(se[:, C:] == -7.0), "a store into the pitch"
                res[f"{kernel}_th_{no}"] = th[:, :C]
                res[f"{kernel}_se_{no}"] = se[:, :C]
            finally:
                for b in bufs:
                    b.free()
                plan.destroy()
    np.savez(out_path, **res)


def host_records():
    recs = [(name, doy_of(a, b)) for name, a, b in RECORDS]
    recs += [(f"{y}y_from_1980", doy_of("1980-01-01", f"{1980 + y}-01-01")) for y in HOST_YEARS]
    # no leap year at all: a 365-day calendar, and the no-leap 6-hourly tstep axis (1,460 labels a year)
    d365 = np.arange(40 * 365) % 365 + 1
    recs.append(("noleap_daily", np.where(d365 >= 60, d365 + 1, d365)))
    recs.append(("noleap_6hourly", np.arange(20 * 1460) % 1460 + 1))
    return recs


def run_host(out_path):
    import xmhw_amd.device as dev
    h = dev.hip()
    res = {}
    for name, doy in host_records():
        plan = dev.Plan(doy, 5)
        try:
            res[f"direct_{name}"] = np.array([plan.sorted_direct(C) for C in (1, 65, 1036800)])
            chunks, table, flags = h.plan_sorted_table(plan.handle, 1)
            res[f"chunks_{name}"], res[f"table_{name}"], res[f"flags_{name}"] = chunks, table, flags
            res[f"info_{name}"] = np.array(h.plan_sorted_info(plan.handle, 1036800))
            r = plan.route(np.float32, 0.9, 1036800)
            res[f"route_{name}"] = np.array([repr(r)])
        finally:
            plan.destroy()
    np.savez(out_path, **res)


if __name__ == "__main__":
    root, mode, out = sys.argv[1:4]
    for p in (root, os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    (run_gpu if mode == "gpu" else run_host)(out)
