"""The conditions the synthetic detect-stage cases of tests/detect_cases.py must meet, asserted on the CPU with the
loop oracles alone (oracle/detect_oracle.py, oracle/features_oracle.py), for the very seeds, shapes and parameters
tests/test_gpu_detect_kernels.py runs on the device."""
import numpy as np
import numpy.testing as npt
import pytest

import detect_cases as dc
from xmhw_amd.detect_front import EVENT_COLUMNS

COL = {c: i for i, c in enumerate(EVENT_COLUMNS)}
CASES = dc.gpu_cases()


def test_every_parameter_set_meets_every_length_width_dtype_and_sign():
    assert len(CASES) == len(set(CASES)) == len(dc.TS) * len(dc.PARAMS)
    for p in dc.PARAMS:
        mine = [c for c in CASES if c[4] == p]
        assert sorted(c[0] for c in mine) == sorted(dc.TS)
        assert {c[1] for c in mine} == set(dc.CS)
        assert {(c[2], c[3]) for c in mine} == {(d, s) for d in (np.float32, np.float64) for s in (False, True)}
    for C in dc.CS:
        assert {(c[2], c[3]) for c in CASES if c[1] == C} == {(d, s) for d in (np.float32, np.float64) for s in (False, True)}
    assert {c[0] % 8 for c in CASES} >= {0, 1, 7}
    assert any(c[0] == 300 and c[1] == 257 for c in CASES)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_series_and_climatologies_are_as_described(dtype):
    r = dc.pitched_case(300, 257, dtype, 11, False)
    x, seas, thresh, rows = r["x"], r["seas"], r["thresh"], r["row_of_t"]
    assert x.dtype == dtype and x.shape == (300, 257) and seas.shape == thresh.shape == (37, 257)
    assert rows.dtype == np.int32 and set(rows) == set(range(37)) and rows[0] != 0
    npt.assert_array_equal(rows[37:], rows[:-37])                       # the labels cycle
    gap = thresh - seas
    assert gap.min() >= 0.6 and gap.max() <= 1.0
    free = x[:, len(dc.LETTERS):].astype(np.float64)
    assert 0.01 < np.isnan(free).mean() < 0.03
    a = free - seas[rows][:, len(dc.LETTERS):]
    ok = ~np.isnan(a[1:]) & ~np.isnan(a[:-1])
    rho = np.corrcoef(a[1:][ok], a[:-1][ok])[0, 1]
    assert 0.85 < rho < 0.95
    cold = dc.pitched_case(300, 257, dtype, 11, True)
    npt.assert_array_equal(cold["x"], -x)
    npt.assert_array_equal(cold["thresh"], thresh)
    assert sorted(r["planted"]) == list(dc.LETTERS) and [r["planted"][k]["col"] for k in dc.LETTERS] == list(range(12))
    single = dc.pitched_case(300, 1, dtype, 11, False)
    assert list(single["planted"]) == ["e"] and single["planted"]["e"]["col"] == 0


def test_planted_items_state_the_length_they_need():
    for m, _, gap in dc.PARAMS:
        full = dc.pitched_case(300, 12, np.float64, 3, False, minDuration=m, maxGap=gap)["planted"]
        assert sorted(full) == list(dc.LETTERS)
        for k, item in full.items():
            if k in "abce":                      # whole-series items: they fit every length
                assert item["need_T"] == 1
                continue
            touched = [last for _, last in item["runs"]] + item["nan"]
            assert max(touched) + 1 < item["need_T"] <= 64, k     # a step below the threshold follows the last run
        for T in dc.TS:
            got = dc.pitched_case(T, 12, np.float64, 3, False, minDuration=m, maxGap=gap)["planted"]
            assert sorted(got) == sorted(k for k in full if full[k]["need_T"] <= T), (m, T)


def _events_of(r, c):
    return r["table"][r["offsets"][c]:r["offsets"][c + 1]]


@pytest.mark.parametrize("case", CASES, ids=dc.case_id)
def test_planted_cells_yield_their_events(case):
    T, C, dtype, cold, (m, jg, gap) = case
    r = dc.case_with_oracle(case)
    P = r["planted"]
    total = r["table"].shape[0]
    assert r["offsets"][-1] == total == int(r["counts"].sum())
    npt.assert_array_equal(r["counts"], (r["start"] >= 0).sum(axis=0))
    if T < 64:
        # short series: whatever fits is planted; nothing at all only where no run can reach minDuration
        assert total > 0 or T < m + 1
        return
    assert total >= C / 4
    if C == 1:
        assert list(P) == ["e"]
    else:
        assert sorted(P) == list(dc.LETTERS)
    ev, b = r["events"], r["bthresh"]

    def cell(k):
        return P[k]["col"], _events_of(r, P[k]["col"])

    if "a" in P:
        c, t = cell("a")
        assert b[:, c].all() and t.shape[0] == 1 and t[0, COL["event"]] == 1 and t[0, COL["index_end"]] == T - 1
        c, t = cell("b")
        assert not b[:, c].any() and t.shape[0] == 0
        c, t = cell("c")
        assert np.isnan(r["x"][:, c]).all() and not b[:, c].any() and t.shape[0] == 0
        # (d) the run from step 0: label 1, step 0 itself is not part of the event
        c, t = cell("d")
        assert t.shape[0] == 1 and b[0, c] and ev[0, c] == -1
        assert t[0, COL["event"]] == 1 and t[0, COL["index_start"]] == 1 and t[0, COL["time_start"]] == 1
        assert t[0, COL["index_end"]] == m + 1 and t[0, COL["duration"]] == m + 1
    # (e) the run that reaches the last step
    c, t = cell("e")
    assert t.shape[0] == 1 and t[0, COL["index_end"]] == T - 1 == t[0, COL["time_end"]]
    assert t[0, COL["index_start"]] == T - 1 - m and ev[T - 1, c] == T - 1 - m
    if C == 1:
        return
    # (f) an event that ends on the last step of an 8-step batch, one step, an event from the second step of the next
    c, t = cell("f")
    (s1, e1), (s2, e2) = P["f"]["runs"]
    assert e1 % 8 == 7 and s2 == e1 + 2 and s2 % 8 == 1 and not b[e1 + 1, c]
    if dc.joins(1, jg, gap):
        assert t.shape[0] == 1 and t[0, COL["index_start"]] == s1 and t[0, COL["index_end"]] == e2
        assert (ev[s1:e2 + 1, c] == s1).all()
    else:
        assert t.shape[0] == 2 and ev[e1 + 1, c] == -1
        npt.assert_array_equal(t[:, COL["index_start"]], [s1, s2])
        npt.assert_array_equal(t[:, COL["index_end"]], [e1, e2])
    assert not np.isnan(t[:, COL["rate_onset"]]).any() and not np.isnan(t[:, COL["rate_decline"]]).any()
    # (g) an event that ends on the last step of a batch, the next sample is missing
    c, t = cell("g")
    (s1, e1), = P["g"]["runs"]
    assert t.shape[0] == 1 and t[0, COL["index_end"]] == e1 and e1 % 8 == 7 and np.isnan(r["x"][e1 + 1, c])
    assert not np.isnan(t[0, COL["rate_decline"]])
    # (h) exactly minDuration steps qualify, minDuration - 1 do not
    c, t = cell("h")
    assert t.shape[0] == 1 and t[0, COL["duration"]] == m and t[0, COL["index_start"]] == P["h"]["runs"][0][0]
    if m > 1:
        s, last = P["h"]["runs"][1]
        assert last - s + 1 == m - 1 and b[s:last + 1, c].all() and (ev[s:last + 1, c] == -1).all()
    # (i) maxGap apart: joined (maxGap = 0: one run anyway); maxGap + 1 apart: never
    c, t = cell("i")
    r1, r2, r3, r4 = P["i"]["runs"]
    assert r2[0] - r1[1] - 1 == gap and r4[0] - r3[1] - 1 == gap + 1
    first_pair = 1 if gap == 0 or dc.joins(gap, jg, gap) else 2
    assert t.shape[0] == first_pair + 2
    npt.assert_array_equal(t[-2:, COL["index_start"]], [r3[0], r4[0]])
    npt.assert_array_equal(t[-2:, COL["index_end"]], [r3[1], r4[1]])
    assert t[0, COL["index_start"]] == r1[0] and t[first_pair - 1, COL["index_end"]] == r2[1]
    # (j) a missing sample between two runs, and a missing sample beside a sample below in the next gap
    c, t = cell("j")
    n1, n2 = P["j"]["nan"]
    assert np.isnan(r["x"][[n1, n2], c]).all()
    j1, j2 = dc.joins(1, jg, gap), dc.joins(2, jg, gap)
    assert t.shape[0] == 3 - j1 - j2
    assert (ev[n1, c] >= 0) == j1 and (ev[n2, c] >= 0) == j2 and (ev[n2 + 1, c] >= 0) == j2
    if j1:
        # the missing sample is skipped by the statistics of the event that covers it
        first = t[0]
        steps = np.nonzero(ev[:, c] == first[COL["event"]])[0]
        x64 = (-1.0 if cold else 1.0) * r["x"][steps, c].astype(np.float64)
        rel = x64 - r["seas"][r["row_of_t"][steps], c]
        assert np.isnan(rel).sum() == 1 + j2
        npt.assert_allclose(first[COL["intensity_mean"]], np.nanmean(rel), rtol=1e-12)
    # (k) two equal, adjacent maxima: the first is the peak
    c, t = cell("k")
    t1, t2 = P["k"]["ties"]
    assert t.shape[0] == 1 and t2 == t1 + 1
    x64 = (-1.0 if cold else 1.0) * r["x"][:, c].astype(np.float64)
    rel = x64 - r["seas"][r["row_of_t"], c]
    assert rel[t1] == rel[t2] == np.nanmax(rel)
    assert t[0, COL["time_peak"]] == t1 == t[0, COL["index_peak"]] and t[0, COL["intensity_max"]] == rel[t1]
    # (l) at the threshold and one ulp below: no exceedance; one ulp above: exceedance
    c, t = cell("l")
    want = np.zeros(T, dtype=bool)
    want[P["l"]["up"]] = True
    npt.assert_array_equal(b[:, c].astype(bool), want)
    th = r["thresh"][r["row_of_t"], c]
    x64 = (-1.0 if cold else 1.0) * r["x"][:, c].astype(np.float64)
    npt.assert_array_equal(x64[P["l"]["at"]], th[P["l"]["at"]])
    one = np.dtype(dtype).type(1)
    for key, side in (("up", np.inf), ("down", -np.inf)):
        steps = P["l"][key]
        npt.assert_array_equal(x64[steps], np.nextafter(th[steps].astype(dtype), one * side).astype(np.float64))
    assert t.shape[0] >= 1
