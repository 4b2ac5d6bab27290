"""Synthetic block_average() inputs built directly (not through detect()), so that every class of input the
kernels of csrc/kernels_stats.hip branch on is present by construction, and the list of shapes the GPU tests
run (tests/test_gpu_stats.py); tests/test_stats_cases.py asserts on the CPU that every case holds its classes.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from xmhw_amd.detect_front import EVENT_COLUMNS
from xmhw_amd.stats import _bin_of_t, block_bins

COL = {c: i for i, c in enumerate(EVENT_COLUMNS)}
TIME_COLUMNS = (COL["time_start"], COL["time_peak"], COL["time_end"])
MTIMES = ("time_start", "time_peak", "time_end")
# the columns agg_mhw reads (stats_exact_oracle.EVENT_SOURCE_COLUMNS, asserted equal in test_stats_cases.py)
SOURCE_COLUMNS = [COL[c] for c in ("event", "duration", "intensity_max", "intensity_mean", "intensity_cumulative",
                                   "intensity_mean_relThresh", "intensity_cumulative_relThresh", "severity_mean",
                                   "severity_cumulative", "rate_onset", "rate_decline")]
MARGIN = 30          # events may start up to MARGIN steps before the axis and end up to MARGIN steps behind it

# The axis of the GPU tests: daily steps from 2004-01-04.  Step 1093 is 2007-01-01, so for T = 1094, 1095, 1096 a
# year boundary -- a bin edge -- lies inside the last group of 8 rows (1088..1095) block_time loads at a time,
# in a partial group for 1094 and 1095; T = 1089..1093 end in 2006 with every residue mod 8.
FIRST_DAY = np.datetime64("2004-01-04")
TS = tuple(range(1096 - 7, 1096 + 1))
CS = (1, 63, 255, 256, 257, 600)
COMBOS = ((np.float32, True), (np.float32, False), (np.float64, True), (np.float64, False))     # (ts dtype, with cats)


def years_of_axis(T):
    return ((FIRST_DAY + np.arange(T)).astype("datetime64[Y]").astype(np.int64) + 1970)


def whole_call_cases():
    """(C, T, blockLength, mtime, ts dtype, with cats): C = 257 and 600 against every T, float32 and float64 each
    and cats alternating so that both cats variants meet every T; the small C against the four dtype / cats
    pairings.  Every value of every axis occurs."""
    out = []
    i = 0
    for C in CS[4:]:
        for T in TS:
            for half in (0, 1):
                dtype, with_cats = COMBOS[2 * half + (T + (C == 600) + half) % 2]
                out.append((C, T, 1 + (i // 3) % 2, MTIMES[i % 3], dtype, with_cats))
                i += 1
    for C in CS[:4]:
        for dtype, with_cats in COMBOS:
            out.append((C, TS[(3 * i) % 8], 1 + (i // 3) % 2, MTIMES[i % 3], dtype, with_cats))
            i += 1
    return out


# (C, T, mtime, ts dtype, with cats) of the narrow-period test and (C, T, blockLength, mtime, ts dtype) of the stride test
NARROW_CASES = [(257, 1096, "time_start", np.float32, True), (600, 1094, "time_peak", np.float64, True),
                (257, 1091, "time_end", np.float64, False), (63, 1093, "time_start", np.float32, False)]
STRIDE_CASES = [(257, 1095, 1, "time_peak", np.float32), (63, 1090, 2, "time_end", np.float64),
                (600, 1096, 1, "time_start", np.float64)]
# (C, T, ts dtype) of the test whose edges reach beyond the axis: bins without a single step
WIDE_CASES = [(257, 1093, np.float32), (63, 1096, np.float64)]


def case_id(case):
    C, T, bl, mtime, dtype, with_cats = case
    return f"C{C}-T{T}-bl{bl}-{mtime}-{np.dtype(dtype).name}-{'cats' if with_cats else 'nocats'}"


def seed_of(C, T):
    return 7919 * C + T


def make_case(seed, C, T, years, edges, dtype=np.float64):
    """table (n_events, 31), offsets (C + 1,), ts (T, C) of ``dtype``, cats (T, C) for the calendar year of every
    step and the bin edges:

    * 0 to 40 events per cell, disjoint and in time order, time_start <= time_peak <= time_end as integral
      float64; cell 0, cell C - 1 and about 10 % of the others have none (a single cell, C = 1, keeps its events:
      the table without events has a test of its own); about 3 % of the events are NaT (NaN in all three time
      columns); events near the ends start before step 0 or end at or behind step T;
    * the other columns: normal draws of mixed sign, intensity_max all negative in about a tenth of the cells,
      about 5 % NaN in every source column, rate_onset NaN in every event that touches one chosen bin of about
      8 % of the cells (an all-NaN column in a non-empty group, whichever time column bins the events);
    * ts: mixed sign with 5 % NaN, about 8 % of the cells all negative and 8 % all positive, one bin all NaN in
      about 5 % of the cells; cats drawn from {NaN, -1, 0, 1, 2, 3, 4, 5}.
    """
    rng = np.random.default_rng(seed)
    years = np.asarray(years, dtype=np.int64)
    bins = _bin_of_t(years, np.asarray(edges))
    nb = len(edges) - 1
    n_ev = rng.integers(1, 41, size=C)
    n_ev[rng.random(C) < 0.10] = 0
    if C > 1:
        n_ev[0] = n_ev[C - 1] = 0
    else:
        n_ev[0] = max(int(n_ev[0]), 20)
    offsets = np.concatenate([[0], np.cumsum(n_ev)]).astype(np.int64)
    table = rng.normal(scale=3.0, size=(int(offsets[-1]), len(EVENT_COLUMNS)))
    negative_max = rng.random(C) < 0.10
    nan_onset = rng.random(C) < 0.08
    for c in range(C):
        n = int(n_ev[c])
        if n == 0:
            continue
        rows = table[offsets[c]:offsets[c + 1]]
        marks = np.sort(rng.choice(np.arange(-MARGIN, T + MARGIN), size=2 * n, replace=False))
        start, end = marks[0::2], marks[1::2]
        peak = rng.integers(start, end + 1)
        rows[:, COL["time_start"]], rows[:, COL["time_peak"]], rows[:, COL["time_end"]] = start, peak, end
        rows[:, COL["index_start"]], rows[:, COL["index_peak"]], rows[:, COL["index_end"]] = start, peak, end
        if negative_max[c]:
            rows[:, COL["intensity_max"]] = -np.abs(rows[:, COL["intensity_max"]]) - 0.01
        if nan_onset[c] and nb > 0:
            inside = np.nonzero((peak >= 0) & (peak < T))[0]
            inside = inside[bins[peak[inside]] >= 0]
            if inside.size:
                k = bins[peak[rng.choice(inside)]]
                touch = np.zeros(n, dtype=bool)
                for col in (start, peak, end):
                    ok = (col >= 0) & (col < T)
                    touch[ok] |= bins[col[ok]] == k
                rows[touch, COL["rate_onset"]] = np.nan
    for col in SOURCE_COLUMNS:
        table[rng.random(table.shape[0]) < 0.05, col] = np.nan
    table[np.ix_(rng.random(table.shape[0]) < 0.03, TIME_COLUMNS)] = np.nan

    ts = rng.normal(scale=4.0, size=(T, C))
    sign = rng.random(C)
    ts[:, sign < 0.08] = -np.abs(ts[:, sign < 0.08]) - 0.5
    ts[:, sign > 0.92] = np.abs(ts[:, sign > 0.92]) + 0.5
    ts[rng.random((T, C)) < 0.05] = np.nan
    if nb > 0:
        for c in np.nonzero(rng.random(C) < 0.05)[0]:
            ts[bins == rng.integers(0, nb), c] = np.nan
    cats = rng.choice(np.array([np.nan, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0]), size=(T, C))
    return table, offsets, ts.astype(dtype), cats


@functools.lru_cache(maxsize=4)
def whole_call_inputs(C, T, blockLength, dtype):
    """The inputs of a whole-call case: bins over the whole axis, as block_average() makes them from a series.
    Cached and shared: treat as read-only."""
    years = years_of_axis(T)
    edges = block_bins([years[0], years[-1]], blockLength)
    table, offsets, ts, cats = make_case(seed_of(C, T), C, T, years, edges, dtype)
    for a in (table, offsets, ts, cats, years, edges):
        a.setflags(write=False)
    return dict(table=table, offsets=offsets, ts=ts, cats=cats, years=years, edges=edges)


@functools.lru_cache(maxsize=4)
def narrow_inputs(C, T, dtype):
    """Bins that cover only the middle year of the axis (2005): steps and events before and behind it are in no bin."""
    years = years_of_axis(T)
    edges = np.array([2005, 2006], dtype=np.int64)
    table, offsets, ts, cats = make_case(seed_of(C, T) + 1, C, T, years, edges, dtype)
    for a in (table, offsets, ts, cats, years, edges):
        a.setflags(write=False)
    return dict(table=table, offsets=offsets, ts=ts, cats=cats, years=years, edges=edges)


@functools.lru_cache(maxsize=2)
def wide_inputs(C, T, dtype):
    """Yearly bins from the year before the axis to two years behind it: the first bin and the last two hold no step
    (and so no event), and nothing ever visits them."""
    years = years_of_axis(T)
    edges = np.arange(years[0] - 1, years[-1] + 4, dtype=np.int64)
    table, offsets, ts, cats = make_case(seed_of(C, T) + 2, C, T, years, edges, dtype)
    for a in (table, offsets, ts, cats, years, edges):
        a.setflags(write=False)
    return dict(table=table, offsets=offsets, ts=ts, cats=cats, years=years, edges=edges)
