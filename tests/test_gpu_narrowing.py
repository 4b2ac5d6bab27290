"""The give-up of the three narrowing ring kernels, at the edges (tests/narrowing_cases.py makes the inputs,
tests/test_narrowing_cases.py checks them on the oracle).

A float64 clim_raw() queues: the sparse probe, a NARROWING float32 ring kernel that reads the doubles as float32 and sets
the plan's flag at the first sample float32 cannot hold, and a GATED float64 kernel that runs only if the flag is set.
Here the series is float32-representable but for ONE sample on a row the probe does not read, so only the row loop of
the narrowing kernel can find it -- on each of the twelve (narrowing -> gated) kernel pairs the default dispatch has,
at the first and last steps and tracks, Feb 29, the padded last lane's track, a chunk's warm-up and first rows, the first
cell, the last cell and the ragged last wave; with a sample an ulp off a float32, out of float32's range at either end,
or the selected extreme of its pools itself.

What a lost check would do (worked out on the source, not by running it): without its `lossy |=` line a narrowing kernel
finishes on the rounded samples and leaves the flag clear; the gated kernel then returns at its first line.  In
test_hidden_sample_ends_on_the_gated_kernel `plan.narrowed()` then answers True (first assertion after the call), and for
kind "top" with q = 1 every row whose pool holds the sample carries float32(v) where the oracle and the narrowing=False
call carry the double v: the bit comparison of thresh and the exact-double rows fail; for "huge" / "above_max" the rows
are inf, for "ulp" / "tiny" the pooled mean moves by more than the tolerance only where the pool is small, which is why
"top" runs at every position.  The same holds for a check that misses a position (a first or warm-up row, the row
consumed just before the loop is left, a padded lane, a cell of a ragged wave): only the cases at that position fail.
Each kernel is pinned by records that reach no other narrowing kernel: clim_ring_f32 (kernels_ring.hip) by the 8-, 65-
and 97-year records and w = 2 and 7; clim_ring2_f32 (kernels_ring2.hip) by 17 (layout 10), 21 (layout 8) and 89 years
(layout 12); clim_ring3_f32 (kernels_ring3.hip) by 9 and 13 (layout 22), 25 (layout 21) and 49 years (layout 20).  A gated
kernel that did not run leaves the 0xFF fill of the output buffers (or the narrowing kernel's partial rows) behind.

What these cases found when they were written: every hidden sample was given up on, thresh was right everywhere, but the
gated 64-bit modes of the second- and third-generation kernels returned seas off by 5 to 100 % in the rows after a "huge"
or "above_max" sample had left the ring (the running float64 sum had been absorbed by it; the generic kernel was right).
Both modes now keep the rounding error of their additions (kernels_ring2.hip / kernels_ring3.hip: lerr).

Tolerances: thresh bit for bit (exact selection + numpy's lerp in float64); seas rtol = atol = 1e-12 against the oracle,
as test_clustered_doubles_through_every_dispatchable_float64_kernel (float64 sums in another order)."""
import numpy as np
import numpy.testing as npt
import pytest

import oracle_fast as fast
import narrowing_cases as nc

pytestmark = pytest.mark.gpu

IDS = [r["id"] for r in nc.ROUTES]
BY_YEARS = {(r["w"], r["years"]): r for r in nc.ROUTES}
ONE_PER_KERNEL = [BY_YEARS[5, 8], BY_YEARS[5, 21], BY_YEARS[5, 25]]          # ring1, ring2, ring3 narrowing


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


class Call:
    """one plan with its own output buffers (pitch ldo); run() fills them with 0xFF bytes first, so that a kernel
    that wrote nothing cannot pass on what the call before left there"""

    def __init__(self, dev, doy, w, C, ldo=None, **kw):
        self.dev, self.h, self.C, self.ldo = dev, dev.hip(), C, C if ldo is None else ldo
        self.plan = dev.Plan(doy, w, **kw)
        self.D = self.plan.D
        self.th = dev.DeviceBuffer(8 * self.D * self.ldo)
        self.se = dev.DeviceBuffer(8 * self.D * self.ldo)

    def route(self, dtype, q):
        return self.plan.route(dtype, q, self.C)

    def run(self, d_ts, itemsize, q, cold, ld=None):
        for b in (self.th, self.se):
            self.h.memset(b.ptr, 0xFF, b.nbytes)
        self.dev.clim_raw(self.plan, d_ts, itemsize, self.C, q, cold, self.th, self.se, ld=ld, ldo=self.ldo)
        self.h.stream_sync(0)
        narrowed = self.plan.narrowed()
        return (self.th.to_array((self.D, self.ldo), np.float64), self.se.to_array((self.D, self.ldo), np.float64),
                narrowed)

    def close(self):
        self.th.free()
        self.se.free()
        self.plan.destroy()


def _same(a, b):
    """bit for bit in the sense of the parity tests: equal values, NaN where NaN"""
    return np.array_equal(a, b, equal_nan=True)


def _assert_same(a, b, msg):
    if not _same(a, b):
        npt.assert_array_equal(a, b, err_msg=msg)


def _assert_seas(got, want, msg):
    with np.errstate(invalid="ignore"):
        npt.assert_allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=msg)


def _oracle(x, doy, q, w, cold):
    with np.errstate(invalid="ignore"):
        _, th, se = fast.raw_clim(-x if cold else x, doy, q, w)
    return th, se


def _patch(dev, d_ts, T, ld, t, c, value):
    dev.hip().memcpy_h2d(d_ts.ptr + 8 * (t * ld + c), np.array([value], dtype=np.float64))


# ---- a. a hidden sample ends on the gated kernel -----------------------------------------------------------------

@pytest.mark.parametrize("cold", [False, True], ids=["warm", "cold"])
@pytest.mark.parametrize("route", nc.ROUTES, ids=IDS)
def test_hidden_sample_ends_on_the_gated_kernel(dev, route, cold):
    time, doy = nc.calendar(route)
    T, C, w = time.shape[0], nc.ncells(route), route["w"]
    x = nc.series(T, C, 300 + route["years"])
    rc = nc.cases(route)
    assert len(rc) == 10 * 3 * 2 + 6
    calls = {(n, narrowing): Call(dev, doy, w, C, kernel="auto", narrowing=narrowing, nchunks=n)
             for n in (0, 3) for narrowing in (True, False)}
    d_ts = dev.DeviceBuffer.from_array(x)
    try:
        for (n, narrowing), call in calls.items():
            for q in (0.9, 1.0):
                r = call.route(np.float64, q)
                if narrowing:
                    assert nc.route_pair(r) == (route["narrow"], route["gated"]), r
                else:
                    assert len(r["launches"]) == 1 and not r["launches"][0]["gated"], r
                    assert (r["launches"][0]["family"], r["launches"][0]["layout"]) == route["gated"], r
        print(route["id"], "runs on", nc.route_pair(calls[0, True].route(np.float64, 0.9)))
        base = {q: _oracle(x, doy, q, w, cold) for q in (0.9, 1.0)}
        cols, vals = nc.hidden_columns(x, rc, cold)
        want = {}
        for q in (0.9, 1.0):
            sel = [i for i, case in enumerate(rc) if nc.q_of(case[3]) == q]
            th, se = _oracle(cols[:, sel], doy, q, w, cold)
            for j, i in enumerate(sel):
                want[i] = th[:, j], se[:, j]
        for i, (t, label, c, kind) in enumerate(rc):
            q = nc.q_of(kind)
            th0, se0 = base[q][0].copy(), base[q][1].copy()
            th0[:, c], se0[:, c] = want[i]
            rows = nc.affected_rows(doy, t, w)
            if kind == "top":
                assert (th0[rows, c] == (-vals[i] if cold else vals[i])).all()
            _patch(dev, d_ts, T, C, t, c, vals[i])
            for n in (0, 3):
                msg = f"{route['id']}: {label}, t={t} cell={c} {kind} v={vals[i]!r} q={q} cold={cold} nchunks={n}"
                th1, se1, narrowed = calls[n, True].run(d_ts, 8, q, cold)
                assert narrowed is False, msg + ": the narrowing kernel did not give up"
                th2, se2, _ = calls[n, False].run(d_ts, 8, q, cold)
                _assert_same(th1, th0, msg + " (thresh against the oracle)")
                _assert_same(th1, th2, msg + " (thresh against narrowing=False)")
                if kind == "top":
                    _assert_same(th1[rows, c], np.full(rows.shape[0], -vals[i] if cold else vals[i]), msg + " (the hidden double)")
                _assert_seas(se1, se0, msg + " (seas against the oracle)")
                _assert_seas(se2, se0, msg + " (seas of narrowing=False against the oracle)")
            _patch(dev, d_ts, T, C, t, c, x[t, c])
        # the series is whole again: it narrows
        _, _, narrowed = calls[0, True].run(d_ts, 8, 0.9, False)
        assert narrowed is True
    finally:
        d_ts.free()
        for call in calls.values():
            call.close()


# ---- b. representable specials stay narrowed ------------------------------------------------------------------------

def _with_payload_nans(x):
    x = x.copy()
    pay = np.array([0x7FF0000000000001, 0xFFF8DEADBEEF0001], dtype=np.uint64).view(np.float64)
    assert np.isnan(pay).all()
    x[:, 6] = pay[np.arange(x.shape[0]) % 2]
    return x


@pytest.mark.parametrize("route", nc.ROUTES, ids=IDS)
def test_representable_specials_stay_narrowed(dev, route):
    """NaN (also with payloads, signalling ones included), +-inf, +-0, float32 subnormals and +-FLT_MAX are all held by
    float32: the call stays on the narrowing kernel and equals, bit for bit, the float32 call on the same kernel (the
    plan's layout set to the narrowing launch's); against the float32 call of the automatic layout (the sorted-list
    kernel for 9..48 tracks: another order of the float64 sums) thresh bit for bit and seas to rounding"""
    time, doy = nc.calendar(route)
    T, C, w = time.shape[0], nc.ncells(route), route["w"]
    x = _with_payload_nans(nc.series(T, C, 400 + route["years"]))
    with np.errstate(invalid="ignore"):             # (the signalling NaN of cell 6)
        x32 = x.astype(np.float32)
    d64, d32 = dev.DeviceBuffer.from_array(x), dev.DeviceBuffer.from_array(x32)
    calls = []
    try:
        for n in (0, 3):
            c64 = Call(dev, doy, w, C, kernel="auto", narrowing=True, nchunks=n)
            twin = Call(dev, doy, w, C, kernel="auto", nchunks=n, layout=route["narrow"][1])
            auto = Call(dev, doy, w, C, kernel="auto", nchunks=n)
            calls += [c64, twin, auto]
            for q in (0.9, 1.0):
                assert nc.route_pair(c64.route(np.float64, q)) == (route["narrow"], route["gated"])
                la = twin.route(np.float32, q)["launches"]
                assert len(la) == 1 and (la[0]["family"], la[0]["layout"], la[0]["lanes"]) == route["narrow"], la
                for cold in (False, True):
                    msg = f"{route['id']}: q={q} cold={cold} nchunks={n}"
                    th, se, narrowed = c64.run(d64, 8, q, cold)
                    assert narrowed is True, msg
                    th32, se32, _ = twin.run(d32, 4, q, cold)
                    _assert_same(th, th32, msg + " (thresh, float32 call on the same kernel)")
                    _assert_same(se, se32, msg + " (seas, float32 call on the same kernel)")
                    assert not np.isnan(th[:, [0, 7, C - 1]]).any() and np.isnan(th[:, [1, 6]]).all(), msg
                    tha, sea, _ = auto.run(d32, 4, q, cold)
                    _assert_same(th, tha, msg + " (thresh, float32 call of the automatic layout)")
                    _assert_seas(se, sea, msg + " (seas, float32 call of the automatic layout)")
    finally:
        d64.free()
        d32.free()
        for call in calls:
            call.close()


# ---- c. pitched input ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ONE_PER_KERNEL, ids=[r["id"] for r in ONE_PER_KERNEL])
def test_pitched_input_with_lossy_padding_stays_narrowed(dev, route):
    """ld = C + 5 with padding columns full of doubles float32 cannot hold, ldo = C + 3: no lane reads the padding
    (dead lanes of the second- and third-generation kernels point at the last live column, those of the first load
    nothing; the probe stops at C), so the call narrows and equals the dense one; the output padding is untouched"""
    time, doy = nc.calendar(route)
    T, C, w = time.shape[0], nc.ncells(route), route["w"]
    x = nc.series(T, C, 500 + route["years"])
    ld, ldo = C + 5, C + 3
    xp = np.empty((T, ld))
    xp[:, :C] = x
    xp[:, C:] = np.where(np.arange(T)[:, None] % 2 == 0, np.pi, 1e300)
    d_x, d_xp = dev.DeviceBuffer.from_array(x), dev.DeviceBuffer.from_array(xp)
    calls = []
    try:
        for n in (0, 3):
            dense = Call(dev, doy, w, C, kernel="auto", narrowing=True, nchunks=n)
            pitched = Call(dev, doy, w, C, ldo=ldo, kernel="auto", narrowing=True, nchunks=n)
            calls += [dense, pitched]
            assert nc.route_pair(pitched.route(np.float64, 0.9)) == (route["narrow"], route["gated"])
            for cold in (False, True):
                msg = f"{route['id']}: cold={cold} nchunks={n}"
                th, se, narrowed = dense.run(d_x, 8, 0.9, cold)
                assert narrowed is True, msg
                thp, sep, narrowed = pitched.run(d_xp, 8, 0.9, cold, ld=ld)
                assert narrowed is True, msg + " (pitched)"
                _assert_same(thp[:, :C], th, msg)
                _assert_same(sep[:, :C], se, msg)
                sentinel = np.full((pitched.D, ldo - C), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
                for out in (thp, sep):
                    npt.assert_array_equal(np.ascontiguousarray(out[:, C:]).view(np.uint64), sentinel, err_msg=msg)
                # ... and a sample hidden in the last live column, next to the padding, is still found
                t = nc.positions(doy, route["years"])[1][0]
                v = nc.checked_value(x, t, C - 1, "top", cold)
                _patch(dev, d_xp, T, ld, t, C - 1, v)
                thh, _, narrowed = pitched.run(d_xp, 8, 1.0, cold, ld=ld)
                _patch(dev, d_xp, T, ld, t, C - 1, x[t, C - 1])
                assert narrowed is False, msg
                rows = nc.affected_rows(doy, t, w)
                _assert_same(thh[rows, C - 1], np.full(rows.shape[0], -v if cold else v), msg + " (the hidden double)")
    finally:
        d_x.free()
        d_xp.free()
        for call in calls:
            call.close()


# ---- d. one plan: lossy, representable, lossy -----------------------------------------------------------------------

@pytest.mark.parametrize("route", ONE_PER_KERNEL, ids=[r["id"] for r in ONE_PER_KERNEL])
def test_one_plan_lossy_representable_lossy(dev, route):
    """the probe clears the plan's flag: what one call found does not decide the next"""
    time, doy = nc.calendar(route)
    T, C, w = time.shape[0], nc.ncells(route), route["w"]
    x = nc.series(T, C, 600 + route["years"])
    pos = nc.positions(doy, route["years"])
    lossy_a = nc.hide(x, pos[3][0], 0, "top")
    lossy_b = nc.hide(x, pos[7][0], C - 1, "ulp")
    call = Call(dev, doy, w, C, kernel="auto", narrowing=True)
    bufs = [dev.DeviceBuffer.from_array(a) for a in (lossy_a, x, lossy_b)]
    try:
        answers = []
        for arr, d_ts in zip((lossy_a, x, lossy_b), bufs):
            th, se, narrowed = call.run(d_ts, 8, 1.0, False)
            answers.append(narrowed)
            th0, se0 = _oracle(arr, doy, 1.0, w, False)
            _assert_same(th, th0, f"{route['id']}: call {len(answers)}")
            _assert_seas(se, se0, f"{route['id']}: call {len(answers)}")
        assert answers == [False, True, False]
    finally:
        for b in bufs:
            b.free()
        call.close()


# ---- e. slabs, f. the public path ------------------------------------------------------------------------------------

@pytest.fixture()
def plans(monkeypatch, dev):
    """records, for every plan the library creates, its float64 route and what narrowed() answers when it is destroyed
    (that is: after its last call)"""
    seen = []
    real = dev.Plan

    class Recording(real):
        def destroy(self):
            if getattr(self, "handle", 0):
                seen.append((nc.route_pair(self.route(np.float64, 1.0, 16)), self.narrowed()))
            super().destroy()

    monkeypatch.setattr(dev, "Plan", Recording)
    return seen


def _check_finished(got, x, doy, t, c, v, **kw):
    """as test_gpu_parity_f64._check: labels, NaN pattern, thresh and seas at rtol 1e-12 -- and the hidden double itself in
    the rows whose pool holds it (not doy 60, a 3-point mean)"""
    d1, t1, s1 = got
    d0, t0, s0 = fast.threshold_cells_fast(x, doy, **kw)
    npt.assert_array_equal(d1, d0)
    npt.assert_array_equal(np.isnan(t1), np.isnan(t0))
    with np.errstate(invalid="ignore"):
        npt.assert_allclose(t1, t0, rtol=1e-12, atol=0, equal_nan=True)
        npt.assert_allclose(s1, s0, rtol=1e-12, atol=0, equal_nan=True)
    rows = nc.affected_rows(doy, t, kw.get("windowHalfWidth", 5))
    rows = rows[d0[rows] != 60]
    assert rows.shape[0] >= 5
    npt.assert_array_equal(t1[rows, c], np.full(rows.shape[0], v))
    npt.assert_array_equal(t0[rows, c], np.full(rows.shape[0], v))


@pytest.mark.parametrize("where", ["last batch", "first batch"])
def test_slabs_find_the_hidden_sample_in_their_own_batch(dev, plans, where):
    route = BY_YEARS[5, 25]
    time, doy = nc.calendar(route)
    T, C = time.shape[0], 70
    x0 = nc.series(T, C, 700)
    c = C - 1 if where == "last batch" else 0
    t = nc.positions(doy, 25)[6][0]
    x = nc.hide(x0, t, c, "top")
    got = dev.calc_clim_device(x, doy, 100, 5, False, 31, False, max_batch_bytes=16 * T * 8)        # 16 cells a batch: 5 batches
    _check_finished(got, x, doy, t, c, x[t, c], pctile=100, smoothPercentile=False)
    # the flag is per call: the last batch decides what the plan answers at the end
    assert plans == [((route["narrow"], route["gated"]), where != "last batch")], plans


def test_threshold_on_a_float64_grid_finds_the_hidden_sample(dev, plans):
    """threshold() on a float64 GridSeries with land: mask, compaction, the three launches, finish, scatter"""
    from xmhw_amd import GridSeries, threshold
    route = BY_YEARS[5, 25]
    time, doy = nc.calendar(route)
    T, nlat, nlon = time.shape[0], 5, 8
    x = nc.series(T, nlat * nlon, 800)
    x[:, [9, 17, 30]] = np.nan                                  # land (with series()'s own all-NaN cell 1)
    ocean = ~np.isnan(x).all(axis=0)
    c = 39
    t = nc.positions(doy, 25)[2][0]
    x = nc.hide(x, t, c, "top")
    grid = GridSeries(x.reshape(T, nlat, nlon), ("time", "lat", "lon"),
                      {"time": time, "lat": np.arange(nlat, dtype=np.float64), "lon": np.arange(nlon, dtype=np.float64)},
                      time_encoding={"calendar": "proleptic_gregorian"})
    ds = threshold(grid, pctile=100, smoothPercentile=False)
    assert ds["thresh"].shape == (366, nlat, nlon)              # no whole grid line is land
    got = (np.asarray(ds.coords["doy"]), np.asarray(ds["thresh"]).reshape(366, -1)[:, ocean],
           np.asarray(ds["seas"]).reshape(366, -1)[:, ocean])
    assert np.isnan(np.asarray(ds["thresh"]).reshape(366, -1)[:, ~ocean]).all()
    _check_finished(got, x[:, ocean], doy, t, int(ocean[:c].sum()), x[t, c], pctile=100, smoothPercentile=False)
    assert plans == [((route["narrow"], route["gated"]), False)], plans


# ---- g. random -----------------------------------------------------------------------------------------------------------

# the rows of the default dispatch's table: (w, track counts)
TABLE = [(5, range(1, 9)), (5, range(9, 13)), (5, list(range(13, 17)) + [19, 20]), (5, range(17, 19)),
         (5, list(range(21, 25)) + list(range(33, 37)) + list(range(45, 49))), (5, list(range(25, 33)) + list(range(37, 45))),
         (5, list(range(49, 65)) + list(range(81, 89))), (5, range(65, 81)), (5, range(89, 97)), (5, range(97, 193)),
         (1, range(1, 49)), (2, range(1, 49)), (3, range(1, 49)), (4, range(1, 49)),
         (7, range(1, 65)), (10, range(1, 49)), (15, range(1, 33))]
MAX_SAMPLES = 97 * 366 * 40                # the largest input of this module


def random_draw(rng):
    """one draw: (doy, w, x with 1..3 hidden samples, the hidden (t, c, kind), C, nchunks, cold, q)"""
    w, tracks = TABLE[int(rng.integers(len(TABLE)))]
    years = int(list(tracks)[int(rng.integers(len(tracks)))])
    time, doy = nc._daily(nc.Y0, nc.Y0 + years - 1)
    T = time.shape[0]
    C = int(min(rng.integers(1, 91), max(MAX_SAMPLES // T, 1)))
    nchunks = int(rng.choice([0, 1, 3, 7]))
    cold = bool(rng.integers(2))
    q = float(rng.choice([0.9, 0.86, 1.0]))
    x = nc.series(T, C, int(rng.integers(1 << 30)))
    probe = set(nc.probe_rows(T))
    hidden = []
    for _ in range(int(rng.integers(1, 4))):
        kind = nc.KINDS[int(rng.integers(len(nc.KINDS)))]
        pool = nc.ordinary_cells(C) if kind in ("top", "ulp") else list(range(C))
        c = int(pool[int(rng.integers(len(pool)))])
        t = int(rng.integers(T))
        while t in probe:
            t = int(rng.integers(T))
        hidden.append((t, c, kind))
    y = x
    for t, c, kind in hidden:
        y = nc.hide(y, t, c, kind, cold) if nc.representable(y[t:t + 1, c])[0] else y      # (two draws on one sample: the first stays)
    return doy, w, y, hidden, C, nchunks, cold, q


@pytest.mark.parametrize("seed", [71, 72])
def test_random_hidden_samples_equal_the_generic_kernel_and_the_oracle(dev, seed):
    rng = np.random.default_rng(seed)
    families, accepted = set(), 0
    while accepted < 16:
        doy, w, x, hidden, C, nchunks, cold, q = random_draw(rng)
        call = Call(dev, doy, w, C, kernel="auto", narrowing=True, nchunks=nchunks)
        generic = None
        d_ts = None
        try:
            la = call.route(np.float64, q)["launches"]
            if not (la and la[0]["narrows"]):          # (no narrowing launch for this plan: not a case of this test)
                continue
            accepted += 1
            families.add(la[0]["family"])
            msg = (f"seed {seed} draw {accepted}: w={w} T={x.shape[0]} C={C} nchunks={nchunks} cold={cold} q={q} hidden={hidden} "
                   f"route={[(l['family'], l['layout'], l['lanes']) for l in la]}")
            generic = Call(dev, doy, w, C, kernel="generic")
            d_ts = dev.DeviceBuffer.from_array(x)
            th, se, narrowed = call.run(d_ts, 8, q, cold)
            assert narrowed is False, msg
            thg, seg, _ = generic.run(d_ts, 8, q, cold)
            _assert_same(th, thg, msg + " (thresh against the generic kernel)")
            _assert_seas(se, seg, msg + " (seas against the generic kernel)")
            # the oracle on the affected cells and a few more
            some = sorted({c for _, c, _ in hidden} | set(rng.integers(0, C, 6).tolist()))
            th0, se0 = _oracle(x[:, some], doy, q, w, cold)
            _assert_same(th[:, some], th0, msg + " (thresh against the oracle)")
            _assert_seas(se[:, some], se0, msg + " (seas against the oracle)")
        finally:
            if d_ts is not None:
                d_ts.free()
            if generic is not None:
                generic.close()
            call.close()
    assert families == {"ring1", "ring2", "ring3"}, families
