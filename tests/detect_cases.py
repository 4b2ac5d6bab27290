"""Synthetic detect-stage inputs with planted cells, the list of cases the GPU tests run on them
(tests/test_gpu_detect_kernels.py) and what the loop oracles make of every case; tests/test_detect_cases.py asserts on
the CPU, under the oracles alone, that the planted cells produce the events they are planted for.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import detect_oracle as det
import features_oracle as fo

# (minDuration, joinGaps, maxGap).  A gap has at least one step, so joinGaps with maxGap = 0 never joins anything.
PARAMS = ((5, True, 2), (3, False, 0), (1, True, 0), (2, True, 1))
# T: around the 8-step batches of detect_events / event_stats / event_intermediate and the 64-step words of the bit
# path; C: one cell, and one past the 128-thread block of event_stats and the 256-thread block of the other kernels
TS = (1, 2, 7, 8, 9, 63, 64, 65, 129, 300)
CS = (1, 129, 257)
LETTERS = "abcdefghijkl"
ROW_SHIFT = 5           # step 0 does not carry climatology row 0


def gpu_cases():
    """(T, C, ts dtype, cold, (minDuration, joinGaps, maxGap)): every parameter set meets every T once; C, the dtype
    and warm / cold cycle with i + j, so that every set also meets every C, both dtypes and both signs, and every C
    meets both dtypes and both signs (3 and 4 are coprime, i + j runs over 0..12)."""
    out = []
    for i, T in enumerate(TS):
        for j, p in enumerate(PARAMS):
            k = (i + j) % 4
            out.append((T, CS[(i + j) % 3], (np.float32, np.float64)[k % 2], bool(k // 2), p))
    return out


def case_id(case):
    T, C, dtype, cold, (m, jg, gap) = case
    return f"T{T}-C{C}-{np.dtype(dtype).name}-{'cold' if cold else 'warm'}-m{m}-{'join' if jg else 'nojoin'}-g{gap}"


def seed_of(case):
    T, C, _, _, (m, _, gap) = case
    return 104729 * T + 31 * C + 7 * m + gap


def joins(gap_steps, joinGaps, maxGap):
    """are two selected events ``gap_steps`` (>= 1) steps apart joined? (identify.py:309-323)"""
    return bool(joinGaps) and 1 <= gap_steps <= maxGap


def pitched_case(T, C, dtype, seed, cold, minDuration=5, maxGap=2):
    """dict(x (T, C) of ``dtype``, seas, thresh (D, C) float64, row_of_t (T,) int32, planted):

    * x: AR(1) anomalies (rho = 0.9) on a small seasonal cycle, about 2 % NaN; D = min(T, 37) climatology rows whose
      labels cycle along time; thresh - seas in [0.6, 1.0].  With ``cold`` the series is negated (the climatologies
      are those of the negated series, as threshold(coldSpells=True) hands them over), so the same events come out.
    * planted: letter -> dict(col, need_T, runs [(first, last) step of each run of exceedances], nan [steps], ...) of
      the planted cells, which are the first columns (C >= 12), in the order of LETTERS; a single cell (C = 1) is
      cell (e).  An item whose ``need_T`` is above T is left out and its column keeps the random series.  The runs
      depend on minDuration (m) and maxGap (g):
      (a) always above, (b) never above, (c) all NaN;
      (d) a run from step 0 (label 1, first step not part of the event: the fillna(0) quirk);
      (e) a run that reaches step T - 1;
      (f) a run ending at step 23 = 8 k - 1, one step below, a run from step 25 = 8 k + 1;
      (g) a run ending at step 47 = 8 k + 7, step 48 NaN;
      (h) a run of exactly m steps and a run of m - 1;
      (i) two runs g steps apart (g = 0: one run) and two runs g + 1 steps apart;
      (j) three runs: a single NaN step between the first two, a NaN step and a step below between the last two;
      (k) a flat climatology and a run whose two highest samples are equal and adjacent (``ties``);
      (l) samples equal to thresh (``at``), one ulp of ``dtype`` above (``up``: the runs) and below (``down``);
          the thresholds of this column are float32 values.
    """
    m, g = int(minDuration), int(maxGap)
    dtype = np.dtype(dtype)
    if not (C == 1 or C >= len(LETTERS)):
        raise ValueError("C must be 1 or at least 12")
    rng = np.random.default_rng(seed)
    D = min(T, 37)
    row_of_t = ((np.arange(T) + ROW_SHIFT) % D).astype(np.int32)
    d = np.arange(D)[:, None]
    seas = 15.0 + 0.5 * np.sin(2 * np.pi * (d / D + rng.random(C)))
    thresh = seas + rng.uniform(0.6, 1.0, size=(D, C))
    cols = {"e": 0} if C == 1 else {k: i for i, k in enumerate(LETTERS)}
    if "k" in cols:
        seas[:, cols["k"]], thresh[:, cols["k"]] = 14.5, 15.25
    if "l" in cols:
        thresh[:, cols["l"]] = thresh[:, cols["l"]].astype(np.float32).astype(np.float64)
        seas[:, cols["l"]] = thresh[:, cols["l"]] - 0.75
    e = rng.normal(size=(T, C))
    anom = np.empty((T, C))
    anom[0] = e[0] * 0.6 / np.sqrt(1 - 0.81)
    for t in range(1, T):
        anom[t] = 0.9 * anom[t - 1] + 0.6 * e[t]
    y = seas[row_of_t] + anom
    y[rng.random((T, C)) < 0.02] = np.nan
    y = y.astype(dtype)

    def above(col, t):
        return thresh[row_of_t[t], col] + 0.25 + 0.5 * rng.random(np.shape(t))

    def below(col, t):
        return seas[row_of_t[t], col] - 0.25 - 0.5 * rng.random(np.shape(t))

    planted = {}

    def plant(letter, need_T, runs, nan=(), **more):
        if letter not in cols or T < need_T:
            return None
        col = cols[letter]
        every = np.arange(T)
        y[:, col] = below(col, every)
        for s, last in runs:
            t = np.arange(s, last + 1)
            y[t, col] = above(col, t)
        for t in nan:
            y[t, col] = np.nan
        planted[letter] = dict(col=col, need_T=need_T, runs=[(int(s), int(last)) for s, last in runs],
                               nan=[int(t) for t in nan], **more)
        return col

    plant("a", 1, [(0, T - 1)])
    plant("b", 1, [])
    plant("c", 1, [], nan=range(T))
    plant("d", m + 3, [(0, m + 1)])
    plant("e", 1, [(max(0, T - 1 - m), T - 1)])
    plant("f", 28 + m, [(22 - m, 23), (25, 26 + m)])
    plant("g", 50, [(46 - m, 47)], nan=[48])
    plant("h", 30 + m, [(10, 9 + m)] + ([(30, 28 + m)] if m > 1 else []))
    r1 = (4, 4 + m)
    r2 = (r1[1] + g + 1, r1[1] + g + 1 + m)
    r3 = (r2[1] + 7, r2[1] + 7 + m)
    r4 = (r3[1] + g + 2, r3[1] + g + 2 + m)
    plant("i", r4[1] + 2, [r1, r2, r3, r4])
    plant("j", 17 + 3 * m, [(10, 10 + m), (12 + m, 12 + 2 * m), (15 + 2 * m, 15 + 3 * m)], nan=[11 + m, 13 + 2 * m])
    col = plant("k", 17 + m, [(12, 15 + m)], ties=[14, 15])
    if col is not None:
        y[14, col] = y[15, col] = 18.5            # above() stays below 16.0: the two highest, exactly equal
    up = list(range(8, 9 + m)) + list(range(10 + m, 11 + 2 * m)) + [12 + 2 * m]
    at, down = [9 + m], [11 + 2 * m]
    col = plant("l", 14 + 2 * m, [(8, 8 + m), (10 + m, 10 + 2 * m), (12 + 2 * m, 12 + 2 * m)], up=up, at=at, down=down)
    if col is not None:
        th = thresh[row_of_t, col].astype(dtype)             # exact: float32 values
        y[at, col] = th[at]
        y[up, col] = np.nextafter(th[up], dtype.type(np.inf))
        y[down, col] = np.nextafter(th[down], dtype.type(-np.inf))
    x = -y if cold else y
    return dict(x=x, seas=seas, thresh=thresh, row_of_t=row_of_t, planted=planted)


def _int_or_minus_one(a):
    return np.where(np.isnan(a), -1, a).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case_with_oracle(case):
    """pitched_case() of a gpu_cases() entry plus what the loop oracles return for it, cell by cell: bthresh (T, C)
    uint8; events, start, end (T, C) int32 with -1 for NaN; counts (C,) int32; offsets (C + 1,) int64; table
    (n_events, 31); inter (8, T, C) float64 and dur (4, T, C) uint8 in the plane order of the event_intermediate
    kernel.  Cached and shared: treat as read-only."""
    from xmhw_amd.detect_front import INTERMEDIATE_F64, INTERMEDIATE_U8
    T, C, dtype, cold, (m, jg, gap) = case
    r = pitched_case(T, C, dtype, seed_of(case), cold, minDuration=m, maxGap=gap)
    x, seas, thresh, rows = r["x"], r["seas"], r["thresh"], r["row_of_t"]
    b = np.zeros((T, C), dtype=np.uint8)
    ev, st, en = (np.empty((T, C), dtype=np.int32) for _ in range(3))
    inter = np.empty((len(INTERMEDIATE_F64), T, C))
    dur = np.empty((len(INTERMEDIATE_U8), T, C), dtype=np.uint8)
    tables = []
    for c in range(C):
        xc = x[:, c].astype(np.float64)
        bc, s0, e0, ev0 = det.detect_front(xc, thresh[:, c], rows, m, jg, gap, coldSpells=cold)
        b[:, c], st[:, c], en[:, c], ev[:, c] = bc, _int_or_minus_one(s0), _int_or_minus_one(e0), _int_or_minus_one(ev0)
        tc = -xc if cold else xc
        with np.errstate(invalid="ignore"):
            tables.append(fo.event_table(tc, seas[rows, c], thresh[rows, c], s0, e0, ev0))
            ic = fo.intermediate_columns(tc, seas[rows, c], thresh[rows, c], ev0)
        for k, name in enumerate(INTERMEDIATE_F64):
            inter[k, :, c] = ic[name]
        for k, name in enumerate(INTERMEDIATE_U8):
            dur[k, :, c] = ic[name]
    counts = np.array([t.shape[0] for t in tables], dtype=np.int32)
    offsets = np.zeros(C + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    r.update(bthresh=b, events=ev, start=st, end=en, counts=counts, offsets=offsets,
             table=np.concatenate(tables, axis=0), inter=inter, dur=dur)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r
