"""The generator of tests/test_gpu_narrowing.py on the oracle (CPU, no GPU), so that the GPU test cannot pass for the
wrong reason: a hidden sample must change the oracle's answer against the float32-rounded series, a "top" sample must be
the threshold of its rows bit for bit, no sample may sit on a row the probe reads, and every record must take the
(narrowing -> gated) kernel pair it is there for (xmhw_plan_route: host code, needs only the built library)."""
import numpy as np
import numpy.testing as npt
import pytest

import oracle_fast as fast
import narrowing_cases as nc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rounded(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("route", nc.ROUTES, ids=[r["id"] for r in nc.ROUTES])
def test_hidden_samples_change_the_oracle_and_top_is_the_threshold(route):
    time, doy = nc.calendar(route)
    T, C, w = time.shape[0], nc.ncells(route), route["w"]
    x = nc.series(T, C, 300 + route["years"])
    cs = nc.cells(C, route["narrow"][2])
    assert len(cs) == 3
    rc = nc.cases(route, kinds_everywhere=("top", "huge"), kinds_twice=())
    assert len(rc) == 2 * 3 * 10
    for cold in (False, True):
        sign = -1.0 if cold else 1.0
        _, base, _ = fast.raw_clim(sign * x[:, cs], doy, 1.0, w)
        cols, vals = nc.hidden_columns(x, rc, cold)
        _, th, se = fast.raw_clim(sign * cols, doy, 1.0, w)
        _, th32, se32 = fast.raw_clim(sign * _rounded(cols), doy, 1.0, w)
        for i, (t, label, c, kind) in enumerate(rc):
            msg = f"{label} t={t} cell={c} {kind} cold={cold}"
            rows = nc.affected_rows(doy, t, w)
            assert w + 1 <= rows.shape[0] <= 2 * w + 1, msg           # (w + 1: the first and the last steps of the record)
            assert (th[:, i] != th32[:, i]).any(), msg                # float32 samples give another threshold
            other = np.setdiff1d(np.arange(th.shape[0]), rows)
            npt.assert_array_equal(_bits(th[other, i]), _bits(base[other, cs.index(c)]), err_msg=msg)
            # both kinds are the selected extreme of every pool that holds them
            npt.assert_array_equal(_bits(th[rows, i]), _bits(np.full(rows.shape[0], sign * vals[i])), err_msg=msg)
            if kind == "top":
                assert abs(vals[i]) < 100 and (th32[rows, i] != sign * vals[i]).all(), msg
        # the columns are what hide() makes
        t, label, c, kind = rc[7]
        npt.assert_array_equal(_bits(nc.hide(x, t, c, kind, cold)[:, c]), _bits(cols[:, 7]))


def test_series_is_float32_representable_and_holds_the_special_cells():
    x = nc.series(3000, 70, 5)
    assert x.dtype == np.float64 and nc.representable(x).all()
    assert np.isnan(x[:, 1]).all() and np.isinf(x[100:140, 2]).all()
    assert (x[:, 3] == 0).all() and np.signbit(x[:, 3]).any() and not np.signbit(x[:, 3]).all()
    assert (x[:, 4] > 0).all() and (x[:, 4] < 2.0 ** -126).all()                        # float32 subnormals
    assert set(np.unique(x[:, 5])) == {-nc.FLT_MAX, nc.FLT_MAX}
    frac = np.isnan(x[:, nc.ordinary_cells(70)]).mean()
    assert 0.01 < frac < 0.03
    for C in (1, 2, 5, 6):                                                               # small grids keep what fits
        assert nc.representable(nc.series(400, C, 1)).all()


@pytest.mark.parametrize("route", nc.ROUTES, ids=[r["id"] for r in nc.ROUTES])
def test_positions_are_off_the_probe_rows_and_where_the_labels_say(route):
    time, doy = nc.calendar(route)
    T = time.shape[0]
    probe = set(nc.probe_rows(T))
    assert 32 <= len(probe) <= 64 and 0 in probe
    pos = nc.positions(doy, route["years"])
    assert len(pos) == 10 and len({t for t, _ in pos}) == 10
    by = {label: t for t, label in pos}
    for t, label in pos:
        assert t not in probe, label
    near = lambda t, want: min(abs(int(t) - int(v)) for v in np.atleast_1d(want)) <= 1     # (moved by one step at most)
    assert by["first year, Jan 2"] == 1
    assert by["last step off the probe rows"] >= T - 2
    feb29 = np.nonzero(doy == 60)[0]
    assert near(by["Feb 29, first leap year"], feb29[0]) and near(by["Feb 29, last leap year"], feb29[-1])
    assert near(by["Dec 31 of a leap year (366)"], feb29[0] + 306)
    assert near(by["Mar 1 of the last year"], np.nonzero(doy == 61)[0][-1])
    for off in (-6, -1, 0, 5):
        t = by[f"middle year, doy D*1/3{off:+d}"]
        assert abs(int(doy[t]) - (122 + off)) <= 1


def test_hide_refuses_probe_rows_and_values_float32_holds():
    x = nc.series(2000, 8, 3)
    with pytest.raises(AssertionError):
        nc.hide(x, 0, 0, "top")                      # a probe row
    with pytest.raises(AssertionError):
        nc.hide(x, 2000 // 32 * 3, 0, "ulp")
    with pytest.raises(AssertionError):
        nc.hide(x, 7, 5, "top")                      # FLT_MAX + 1.12 is FLT_MAX again
    for kind in nc.KINDS:
        for cold in (False, True):
            y = nc.hide(x, 7, 0, kind, cold)
            changed = np.argwhere(_bits(y) != _bits(x))
            assert changed.tolist() == [[7, 0]] and not nc.representable(y)[7, 0], kind
    assert nc.hide(x, 7, 0, "above_max")[7, 0] > nc.FLT_MAX
    with np.errstate(over="ignore", under="ignore"):
        assert np.isinf(np.float32(nc.hide(x, 7, 0, "above_max")[7, 0]))
        assert np.float32(nc.hide(x, 7, 0, "tiny")[7, 0]) == 0
    # an all-NaN cell and a NaN sample still take the kinds that do not start from the cell's own values
    assert nc.hide(x, 7, 1, "huge")[7, 1] == 1e300 and nc.hide(x, 7, 1, "tiny", True)[7, 1] == 2.0 ** -150


@pytest.fixture(scope="module")
def plan_type():
    try:
        from xmhw_amd.device import Plan
        from xmhw_amd._lib import hip
        hip()
    except Exception as e:                # noqa: BLE001 -- the host library is not built, or does not load without a GPU
        pytest.skip(f"the host library could not be loaded: {e}")
    return Plan


def test_every_record_takes_the_kernel_pair_it_stands_for(plan_type):
    seen, seen32 = set(), set()
    for route in nc.ROUTES:
        time, doy = nc.calendar(route)
        for nchunks in (0, 3):
            plan = plan_type(doy, route["w"], kernel="auto", narrowing=True, nchunks=nchunks)
            try:
                assert plan.ntracks == route["years"]
                for q in (0.9, 1.0, 0.86):
                    pair = nc.route_pair(plan.route(np.float64, q, nc.ncells(route)))
                    assert pair == (route["narrow"], route["gated"]), (route["id"], q, nchunks, pair)
                # (the float32 call the representable series is compared with)
                seen32.add(plan.route(np.float32, 0.9, nc.ncells(route))["launches"][0]["family"])
            finally:
                plan.destroy()
        seen |= {route["narrow"][0], route["gated"][0]}
    assert len({(r["narrow"], r["gated"]) for r in nc.ROUTES}) == len(nc.ROUTES) == 12
    assert {r["narrow"][:2] for r in nc.ROUTES} >= {("ring1", -1), ("ring2", 8), ("ring2", 10), ("ring2", 12),
                                                    ("ring3", 20), ("ring3", 21), ("ring3", 22)}
    assert seen == {"generic", "ring1", "ring2", "ring3"}           # every family a float64 call can launch ...
    assert seen | seen32 == {"generic", "ring1", "ring2", "ring3", "sorted"}      # ... and with the float32 twin all five
