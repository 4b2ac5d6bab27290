"""The cases of tests/f64_mode_cases.py, checked on the host (no GPU): each expects the instantiation the dispatch sends
its record to, together they reach every dispatchable instantiation of the 64-bit mode at its least and at its most, and
their samples are the hazard they are meant to be -- on the clustered cells at least half of all (doy, cell) rows
bracket their quantile between two different doubles with the same high key word, and no sample is a float32.

The hazard share is a condition on the inputs, not a measurement of the kernels: a selection that ignored the low words
could not tell such a bracket apart.  The bound of 0.5 was set before the generator was written (a generator of this
shape gave 0.81 to 0.83 on whole-year records of 9, 40 and 96 years at q = 0.9); a case that falls short gets another
seed or other levels, never another bound."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import f64_mode_cases as fc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHILD = os.path.join(ROOT, "tests", "f64_mode_child.py")
ROUTE_FAMILIES = ("generic", "ring1", "ring2", "ring3", "ring4", "sorted")      # include/xmhw_amd.h: XMHW_ROUTE_*
ALL = [c for cases in fc.CASES for c in cases]
IDS = [c["id"] for c in ALL]

# the instantiations of the 64-bit mode that some setting of the switches dispatches (include/xmhw_amd.h,
# xmhw_plan_f64_mode) ...
DISPATCHABLE = {("ring2", 12, 16, 1), ("ring2", 12, 16, 4), ("ring2", 12, 16, 5), ("ring2", 12, 16, 6),
                ("ring3", 21, 4, 4), ("ring3", 21, 4, 5),
                ("ring3", 20, 8, 2), ("ring3", 20, 8, 3), ("ring3", 20, 8, 4), ("ring3", 20, 8, 5), ("ring3", 20, 8, 6),
                ("ring2", 8, 8, 2), ("ring2", 8, 8, 3), ("ring2", 8, 8, 4), ("ring2", 8, 8, 5), ("ring2", 8, 8, 6)}
# ... and the one only XMHW_RING3_F64=0 with XMHW_RING2_F64_LDS=0 reaches
TWO_SWITCHES_ONLY = ("ring2", 12, 16, 3)


def child_env(leg):
    """the parent's environment without any switch of the dispatch, with the leg's own"""
    env = {k: v for k, v in os.environ.items()
           if not (k == "XMHW_SORTED" or k.startswith("XMHW_RING2") or k.startswith("XMHW_RING3"))}
    env.update(fc.LEGS[leg])
    return env


def _recorder():
    spec = importlib.util.spec_from_file_location("record_routes", os.path.join(ROOT, "tools", "record_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    """{leg index: {tracks: instantiation}}: the single launch of a float64 call -- w = 5, automatic layout and
    kernel, narrowing off -- as tests/golden/threshold_routes.npz holds it (the same for every quantile)"""
    rec = _recorder()
    out = {}
    with np.load(rec.FIXTURE) as z:
        assert tuple(z["legs"]) == rec.LEGS
        for leg, name in enumerate(fc.RECORDED_AS):
            if name is None:
                continue
            i = rec.LEGS.index(name)
            routes = z[f"{i}_routes"][rec.WINDOWS.index(5) if i == 0 else 0]
            r = routes[:, rec.LAYOUTS.index(None), rec.KERNELS.index(0), 0, rec.ELEM_BYTES.index(8)]    # (tracks, q, words)
            assert (r == r[:, :1]).all()
            out[leg] = {}
            for n in rec.TRACKS:
                status, count, family, layout, lanes, tpl, narrows, gated = (int(v) for v in r[n - 1, 0, :8])
                assert (status, count, narrows, gated) == (0, 1, 0, 0), (name, n)
                out[leg][n] = (ROUTE_FAMILIES[family], layout, lanes, tpl)
    return out


@pytest.fixture(scope="module")
def two_switch_routes(tmp_path_factory):
    """what a process with the last leg's switches answers: the routes of the leg's cases and of 1 .. 96 tracks"""
    leg = len(fc.LEGS) - 1
    assert fc.RECORDED_AS[leg] is None
    out = tmp_path_factory.mktemp("f64_routes") / "routes.npz"
    p = subprocess.run([sys.executable, CHILD, str(leg), str(out), "routes"], env=child_env(leg), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with np.load(out) as z:
        return leg, {k: json.loads(str(z[k])) for k in z.files}


def _instantiation(launch):
    return tuple(launch[:4])


def test_the_legs_are_the_four_of_the_issue():
    assert fc.LEGS == ({}, {"XMHW_RING3_F64": "0"}, {"XMHW_RING3_F64_LANES": "8"},
                       {"XMHW_RING3_F64": "0", "XMHW_RING2_F64_LDS": "0"})
    assert len(fc.CASES) == len(fc.LEGS) == len(fc.RECORDED_AS)
    assert len(set(IDS)) == len(IDS)
    assert len({c["seed"] for c in ALL}) == len(ALL)


IN_FIXTURE = [c for c in ALL if fc.RECORDED_AS[c["leg"]] is not None]      # (the other leg: test_two_switch_leg_routes)


@pytest.mark.parametrize("case", IN_FIXTURE, ids=[c["id"] for c in IN_FIXTURE])
def test_case_expects_the_recorded_route(recorded, case):
    from xmhw_amd.device import Plan
    time, doy = fc.calendar(case)
    plan = Plan(doy, fc.W)
    try:
        assert plan.ntracks == case["tracks"]
    finally:
        plan.destroy()
    assert recorded[case["leg"]][case["tracks"]] == case["expect"]


def test_two_switch_leg_routes(recorded, two_switch_routes):
    from xmhw_amd.device import Plan
    leg, got = two_switch_routes
    for i, case in enumerate(fc.CASES[leg]):
        time, doy = fc.calendar(case)
        plan = Plan(doy, fc.W)
        try:
            assert plan.ntracks == case["tracks"]
        finally:
            plan.destroy()
        off, on = got[f"{i}_route"]["off"], got[f"{i}_route"]["on"]
        assert len(off) == 1 and _instantiation(off[0]) == case["expect"] and off[0][4:] == [0, 0], (case["id"], off)
        assert len(on) == 2 and _instantiation(on[1]) == case["expect"] and on[0][4:] == [1, 0] and on[1][4:] == [0, 1], \
            (case["id"], on)
    # the leg's table, from the child's answers: what the cases' least and most are taken from
    table = {n + 1: _instantiation(la[0]) for n, la in enumerate(got["tracks"])}
    assert all(len(la) == 1 for la in got["tracks"])
    reach = {}
    for n, inst in table.items():
        reach.setdefault(inst, []).append(n)
    one_switch = recorded[1]
    for n in range(1, 97):
        # XMHW_RING2_F64_LDS=0 on top of XMHW_RING3_F64=0 moves the records whose low words would be in LDS, no other
        assert (table[n] != one_switch[n]) == (one_switch[n] in (("ring2", 8, 8, 5), ("ring2", 8, 8, 6))), n
    for case in fc.CASES[leg]:
        want = min(reach[case["expect"]]) if case["kind"] == "least" else max(reach[case["expect"]])
        assert case["tracks"] == want, case["id"]


def test_cases_reach_every_dispatchable_instantiation_at_its_least_and_most(recorded, two_switch_routes):
    leg4, got = two_switch_routes
    tables = dict(recorded)
    tables[leg4] = {n + 1: _instantiation(la[0]) for n, la in enumerate(got["tracks"])}
    reach = {}                                   # instantiation -> every track count some leg sends to it (1 .. 96)
    for table in tables.values():
        for n in range(1, 97):
            reach.setdefault(table[n], set()).add(n)
    want = set(DISPATCHABLE)
    if TWO_SWITCHES_ONLY in reach:
        want.add(TWO_SWITCHES_ONLY)
    assert set(reach) == want
    assert len(DISPATCHABLE) == 16
    for inst in sorted(want):
        least = [c for c in ALL if c["expect"] == inst and c["kind"] == "least" and c["tracks"] == min(reach[inst])]
        most = [c for c in ALL if c["expect"] == inst and c["kind"] == "most" and c["tracks"] == max(reach[inst])]
        assert any(c["q"] == 0.9 and not c["negate"] and c["nchunks"] == 0 and c["whole_years"] for c in least), inst
        assert any(c["q"] == 0.1 and c["negate"] and c["nchunks"] == 3 and not c["whole_years"] for c in most), inst
    # within a leg too: every instantiation the leg reaches runs at the least and the most tracks the leg sends to it,
    # unless an earlier leg runs that very record on it
    for leg, table in tables.items():
        mine = {}
        for n in range(1, 97):
            mine.setdefault(table[n], []).append(n)
        for inst, tracks in mine.items():
            for kind, n in (("least", min(tracks)), ("most", max(tracks))):
                legs = [c["leg"] for c in ALL if c["expect"] == inst and c["kind"] == kind and c["tracks"] == n
                        and tables[c["leg"]][n] == inst]
                assert legs and min(legs) <= leg, (leg, inst, kind, n)
    for leg, cases in enumerate(fc.CASES):
        small = min(c["tracks"] for c in cases)
        assert {c["q"] for c in cases if c["tracks"] == small} >= set(fc.EXTRA_Q), leg
        families = {c["expect"][0] for c in cases}
        assert {c["expect"][0] for c in cases if c["pitched"]} == families, leg
        assert sum(c["pitched"] for c in cases) == len(families), leg
    assert fc.C == 37 and fc.PITCH == dict(ld=fc.C + 3, first=5, ldo=fc.C + 2)


def test_calendar_of_a_most_record_starts_and_ends_inside_a_year():
    case = next(c for c in ALL if c["kind"] == "most")
    time, doy = fc.calendar(case)
    assert str(time[0]) == f"{fc.Y0}-04-17" and str(time[-1]) == f"{fc.Y0 + case['tracks'] - 1}-10-03"
    assert doy[0] == 108 and doy[-1] == 277                 # (the doy labels are those of a leap year)
    case = next(c for c in ALL if c["kind"] == "least")
    time, doy = fc.calendar(case)
    assert str(time[0]) == f"{fc.Y0}-01-01" and str(time[-1]) == f"{fc.Y0 + case['tracks'] - 1}-12-31"


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_inputs_are_the_hazard(case):
    doy, x = fc.samples(case)
    cells = fc.clustered_cells(fc.C)
    assert len(cells) == fc.C - 6
    cl = x[:, cells]
    # no sample of a clustered cell is a float32 (the 1 % NaN are no samples)
    assert not fc.representable(cl[~np.isnan(cl)]).any()
    share = fc.hazard_share(case, cells, x, doy)
    print(case["id"], "hazard share", round(share, 4))
    assert share >= 0.5, share


def test_clustered_samples_are_what_they_claim():
    T = 3 * 365
    x = fc.clustered(T, fc.C, 5)
    assert x.dtype == np.float64 and x.shape == (T, fc.C)
    cells = fc.clustered_cells(fc.C)
    cl = x[:, cells]
    ok = ~np.isnan(cl)
    assert 0.005 < 1 - ok.mean() < 0.015
    # upper half negative, lower half positive
    sign = np.sign(np.where(ok, cl, 0).sum(axis=0))
    assert (sign == np.where(np.array(cells) > fc.C // 2, -1, 1)).all()
    assert (sign < 0).sum() >= 15 and (sign > 0).sum() >= 15
    # every sample shares the high key word of its level; repeats are exact ties
    lev = np.round(np.abs(cl[ok]) / fc.STEP) * fc.STEP
    a = np.abs(cl[ok])
    assert ((fc.keys(a) >> np.uint64(32)) == (fc.keys(lev) >> np.uint64(32))).all()
    assert (a > lev).all() and (a < lev * (1 + 2.0 ** -21)).all()
    rep = a == lev * (1.0 + fc.REPEAT)
    assert 0.13 < rep.mean() < 0.17
    assert np.unique(a[~rep]).shape[0] == (~rep).sum()               # distinct doubles
    # the special cells
    ice = x[:, fc.NEAR_FREEZING]
    ice = ice[~np.isnan(ice)]
    assert (np.abs(ice + 1.8) < 1e-5).all() and np.unique(np.round((ice + 1.8) * 2.0 ** 20)).shape[0] >= 5
    z = x[:, fc.ZEROS]
    z = z[~np.isnan(z)]
    assert set(np.round(z * 1e9).astype(int)) == {-2, -1, 0, 1, 2}
    assert (np.signbit(z[z == 0])).any() and (~np.signbit(z[z == 0])).any()
    assert np.isnan(x[:, fc.ALL_NAN]).all()
    inf = x[:, fc.INFS]
    assert np.isposinf(inf).sum() >= 35 and np.isneginf(inf).sum() >= 2 and np.isneginf(inf).sum() <= 3
    big, tiny = x[:, fc.HUGE], x[:, fc.TINY]
    assert np.nanmin(np.abs(big)) > 1e300 and 0 < np.nanmax(np.abs(tiny)) < 2e-308
    assert np.array_equal(fc.clustered(T, fc.C, 5), x, equal_nan=True)
