"""int16 codes read in place (xmhw_clim_raw_i16: clim_sorted_i16<YPS, K, KL> and its recomputation) against the float64
ORACLE (oracle_fast.raw_clim) on the series xarray would hand the reference (ingest_oracle.decode_cf: float32 attributes
decode in float32, float64 attributes in float64, a _FillValue alone or no attributes to float(code); the fill code -> NaN).
Cold spells: the oracle gets the negated series, as the reference does.

Every packing recipe (float32 / float64 attributes with either sign of scale_factor, fill only, nothing: the kernel's modes
1, 2 and 3), both signs of `negate`, high and mirrored (q <= 0.15) quantiles, both byte orders, every instantiation of the
i16 kernel (5..24 tracks per lane), overflowing lists, fill codes other than -32768, pitched ld / ldo.

What is asserted:
- thresh: bit for bit equal to the oracle, NaN positions included, in every mode.
- seas, mode 3 (no scale / offset): bit for bit equal to the oracle -- the integer sum of the codes and the oracle's
  nansum of integer-valued float64 are both exact, and each is divided once by n.
- seas, mode 2 (float64 attributes): bit for bit equal to oracle_fast.packed_mean_f64, the restatement of what the code
  documents (+-((S / n) * s + o), S the exact integer sum of the valid codes), and within rtol 1e-12 / atol
  1e-13 max|x| of the oracle's mean of the decoded values.
- seas, mode 1 (float32 attributes): bit for bit equal to xmhw_decode + the float32 path (tests/test_gpu_packed.py), and
  within rtol 1e-12 / atol 1e-13 max|x| of the oracle.
"""
import os
import sys

import numpy as np
import numpy.testing as npt
import pytest

import oracle_fast as fast
import xmhw_oracle as ora
from ingest_oracle import decode_cf

pytestmark = pytest.mark.gpu

FILL = -32768
F32 = lambda v: float(np.float32(v))          # noqa: E731

# name -> (scale_factor, add_offset, fill code, decoded dtype, kernel mode).  The offsets put 0 inside the data's range.
RECIPES = {
    "f32_pos": (F32(0.01), F32(1.5), FILL, "float32", 1),
    "f32_neg": (F32(-0.01), F32(1.5), FILL, "float32", 1),
    "f64_pos": (0.01, 1.5, FILL, "float64", 2),
    "f64_neg": (-0.0021973, 0.3, FILL, "float64", 2),
    "fill_only": (None, None, FILL, "float32", 3),
    "none": (None, None, None, "float32", 3),
}
QS = [0.0, 0.013, 0.1, 0.15, 0.85, 0.9, 0.99, 1.0]
BIG_Q = {"f32_pos": 0.9, "f32_neg": 0.013, "f64_pos": 0.1, "f64_neg": 0.99, "fill_only": 0.0, "none": 1.0}
# tracks per lane -> (keys per list, LDS bytes per wave) of kSorted (kernels_sorted.hip)
KSORTED = {5: (6, 8960), 6: (6, 8960), 7: (8, 11520), 8: (8, 11520), 9: (10, 14080), 10: (10, 14080), 11: (10, 14080),
           12: (10, 14080), 13: (12, 17920), 14: (12, 17920), 15: (12, 17920), 16: (12, 17920), 17: (14, 20480),
           18: (14, 20480), 19: (16, 20480), 20: (16, 20480), 21: (18, 23040), 22: (18, 23040), 23: (18, 23040),
           24: (18, 23040)}


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


def _daily(y0, y1, start=None, stop=None):
    time = np.arange(start or f"{y0}-01-01", stop or f"{y1 + 1}-01-01", dtype="datetime64[D]")
    return ora.add_doy(time)


def _gen(T, C, seed, center=(-400, 400), amp=(200, 1000), noise=100.0, fillfrac=0.01):
    """codes of a seasonal series that crosses code 0 (and, with RECIPES' offsets, value 0); fill codes in the first wave
    of 32 cells only.  A fill code anywhere in a wave sends that wave's row to the general path (float64 sums of the
    converted codes); the second wave, free of fill, runs plain rows -- the integer row sums of modes 2 and 3"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    c = rng.uniform(*center, C) + rng.uniform(*amp, C) * np.sin(2 * np.pi * (t - rng.uniform(0, 365, C)) / 365.25) \
        + noise * rng.normal(size=(T, C))
    codes = np.clip(np.rint(c), -32767, 32767).astype(np.int16)
    if fillfrac:
        miss = rng.random((T, C)) < fillfrac
        miss[:, 32:] = False
        codes[miss] = FILL
    return codes


def _decoded(codes, recipe):
    """the series the reference sees (xarray's CF decoding, restated by ingest_oracle.decode_cf), as float64"""
    scale, offset, fill, decoded, _ = recipe
    return decode_cf(codes, dict(scale=scale, offset=offset, fill=fill, out=decoded)).astype(np.float64)


def _launch(dev, codes, doy, q, negate, recipe, big_endian=False, ld=None, ldo=None, sentinel=None):
    """clim_raw_packed on codes (T, C) -- stored in a (T, ld) buffer, results in (D, ldo) buffers, optionally prefilled
    with a sentinel; returns the full (D, ldo) arrays"""
    scale, offset, fill, decoded, _ = recipe
    T, C = codes.shape
    ld = C if ld is None else ld
    ldo = C if ldo is None else ldo
    stored = np.full((T, ld), 12345, dtype=np.int16)
    stored[:, :C] = codes
    if big_endian:
        stored = stored.astype(">i2")
    plan = dev.Plan(doy, 5)
    bufs = []
    try:
        D = plan.D
        d_codes = dev.DeviceBuffer.from_array(np.ascontiguousarray(stored).view(np.int16)); bufs.append(d_codes)
        init = np.full((D, ldo), np.nan if sentinel is None else sentinel)
        th = dev.DeviceBuffer.from_array(init); bufs.append(th)
        se = dev.DeviceBuffer.from_array(init); bufs.append(se)
        dev.clim_raw_packed(plan, d_codes, C, q, negate, th, se, scale_factor=scale, add_offset=offset, fill=fill,
                            decoded=decoded, big_endian=big_endian, ld=ld, ldo=ldo)
        dev.hip().stream_sync(0)
        return th.to_array((D, ldo), np.float64), se.to_array((D, ldo), np.float64)
    finally:
        for b in bufs:
            b.free()
        plan.destroy()


def _float32_path(dev, codes, doy, q, negate, recipe):
    """xmhw_decode + the float32 path on the same codes: mode 1's bit-for-bit referee for seas"""
    scale, offset, fill, _, _ = recipe
    h = dev.hip()
    T, C = codes.shape
    bufs = []
    plan = dev.Plan(doy, 5)
    try:
        d_raw = dev.DeviceBuffer.from_array(codes); bufs.append(d_raw)
        d_ts = dev.DeviceBuffer(4 * T * C); bufs.append(d_ts)
        h.decode(d_raw.ptr, 2, 0, T, C, C, d_ts.ptr, 4, C, True, scale, offset, fill is not None,
                 0.0 if fill is None else float(fill), 0)
        th, se = dev.DeviceBuffer(8 * plan.D * C), dev.DeviceBuffer(8 * plan.D * C)
        bufs += [th, se]
        dev.clim_raw(plan, d_ts, 4, C, q, negate, th, se)
        h.stream_sync(0)
        return th.to_array((plan.D, C), np.float64), se.to_array((plan.D, C), np.float64)
    finally:
        for b in bufs:
            b.free()
        plan.destroy()


def _check(dev, codes, doy, q, negate, recipe, th, se, msg=""):
    """the assertions of the module docstring"""
    scale, offset, fill, _, mode = recipe
    x = _decoded(codes, recipe)
    _, oth, ose = fast.raw_clim(-x if negate else x, doy, q, 5)
    npt.assert_array_equal(th, oth, err_msg=f"thresh {msg}")
    if mode == 3:
        npt.assert_array_equal(se, ose, err_msg=f"seas {msg}")
        return
    with np.errstate(all="ignore"):
        amax = float(np.nanmax(np.abs(x))) if np.isfinite(x).any() else 1.0
    npt.assert_array_equal(np.isnan(se), np.isnan(ose), err_msg=f"seas NaN {msg}")
    npt.assert_allclose(se, ose, rtol=1e-12, atol=1e-13 * amax, err_msg=f"seas vs oracle {msg}")
    if mode == 2:
        npt.assert_array_equal(se, fast.packed_mean_f64(codes, doy, 5, scale, offset, fill=fill, negate=negate),
                               err_msg=f"seas vs restatement {msg}")
    else:
        _, sf = _float32_path(dev, codes, doy, q, negate, recipe)
        npt.assert_array_equal(se, sf, err_msg=f"seas vs float32 path {msg}")


# ---- 1. recipe x sign matrix --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def matrix_data():
    doy = _daily(1982, 2021)
    T, C = doy.shape[0], 45
    codes = _gen(T, C, 101, fillfrac=0.014)                         # 1 % of all samples
    codes[:, 1] = FILL                                               # land
    codes[5000:5100, 2] = FILL                                       # a 100-day gap
    t = np.arange(T)
    season = np.sin(2 * np.pi * t / 365.25)
    for c in (3, 33):                                                # (both waves: general and plain rows)
        codes[:, c] = np.clip(np.rint(31000 + 3000 * season), -32767, 32767)        # at +32767 for part of every year
        codes[:, c + 1] = np.clip(np.rint(-31000 - 3000 * season), -32767, 32767)   # at -32767
    assert (codes[:, 3] == 32767).mean() > 0.1 and (codes[:, 4] == -32767).mean() > 0.1
    return doy, codes


_MATRIX = [(r, q, False) for r in RECIPES for q in QS] + [(r, BIG_Q[r], True) for r in RECIPES]


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("name,q,big_endian", _MATRIX)
def test_recipe_sign_matrix(dev, matrix_data, name, q, big_endian, negate):
    """40 daily years x 45 cells: 1 % fill, a land cell, a 100-day gap, cells saturating at +-32767, codes and values
    crossing 0 -- every recipe, both signs, high and mirrored quantiles (the three sign flips of mode 2 compose).  The
    fill sits in the first wave; the second runs the integer row sums"""
    doy, codes = matrix_data
    recipe = RECIPES[name]
    th, se = _launch(dev, codes, doy, q, negate, recipe, big_endian=big_endian)
    _check(dev, codes, doy, q, negate, recipe, th, se, f"{name} q={q} negate={negate} big={big_endian}")
    if recipe[2] is not None:
        assert np.isnan(th[:, 1]).all() and np.isnan(se[:, 1]).all()
    assert np.isfinite(th[:, 0]).all()


# ---- 2. every instantiation ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("yps", sorted(KSORTED))
def test_every_instantiation(dev, yps):
    """a record of 2 yps or 2 yps - 1 tracks (odd for odd yps: the padded slot of the second lane) reaches
    clim_sorted_i16<yps, K, KL>; mode 3 with fill and mode 2 with a negative scale_factor, q = 0.9 and 0.1"""
    ntracks = 2 * yps - (yps % 2)
    doy = _daily(1975, 1975 + ntracks - 1)
    codes = _gen(doy.shape[0], 45, 200 + yps)
    codes[:, 5] = FILL
    plan = dev.Plan(doy, 5)
    try:
        keys, lds, _ = dev.hip().plan_sorted_info(plan.handle, 45)
        assert (plan.ntracks, int(keys), int(lds)) == (ntracks,) + KSORTED[yps], (plan.ntracks, keys, lds)
        assert plan.layout_in_use() == 40
    finally:
        plan.destroy()
    for i, (name, q) in enumerate((("fill_only", 0.9), ("fill_only", 0.1), ("f64_neg", 0.9), ("f64_neg", 0.1))):
        negate = (yps + i) % 2 == 1
        th, se = _launch(dev, codes, doy, q, negate, RECIPES[name])
        _check(dev, codes, doy, q, negate, RECIPES[name], th, se, f"yps={yps} {name} q={q} negate={negate}")


# ---- 3. lists that overflow ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def steep_data():
    """amplitude 20..30 K in 0.01 K codes (as test_flagged_rows_are_recomputed_from_the_codes), partial first and last year"""
    doy = _daily(0, 0, start="1982-03-17", stop="2021-10-09")
    codes = _gen(doy.shape[0], 48, 303, center=(-500, 500), amp=(2000, 3000), noise=100.0, fillfrac=0.005)
    return doy, codes


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("q", [0.9, 0.1])
@pytest.mark.parametrize("name", ["f32_pos", "f64_neg", "fill_only"])
def test_overflowing_lists_are_recomputed_from_the_codes(dev, steep_data, name, q, negate):
    doy, codes = steep_data
    th, se = _launch(dev, codes, doy, q, negate, RECIPES[name])
    _check(dev, codes, doy, q, negate, RECIPES[name], th, se, f"{name} q={q} negate={negate}")


# ---- 4. edges -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [32767, 0])
@pytest.mark.parametrize("name", ["f32_neg", "f64_pos", "fill_only"])
def test_fill_codes_other_than_the_lowest(dev, name, fill):
    """32767 (the data saturate there) and 0 (inside the data's range) as the fill code; -32768 is then a value"""
    doy = _daily(1991, 2020)
    codes = _gen(doy.shape[0], 40, 400 + fill % 7, fillfrac=0.0)
    codes[:, 3] = np.clip(np.rint(31000 + 3000 * np.sin(2 * np.pi * np.arange(doy.shape[0]) / 365.25)), -32767, 32767)
    codes[::97, 6] = -32768                                          # a value here
    assert (codes == fill).sum() > 100
    recipe = RECIPES[name][:2] + (fill,) + RECIPES[name][3:]
    for q, negate in ((0.9, False), (0.1, True), (0.99, True), (0.013, False)):
        th, se = _launch(dev, codes, doy, q, negate, recipe)
        _check(dev, codes, doy, q, negate, recipe, th, se, f"{name} fill={fill} q={q} negate={negate}")
    assert np.isfinite(th[:, 6]).all() and np.isfinite(se[:, 6]).all()


@pytest.mark.parametrize("name", ["f32_pos", "f64_neg", "none"])
def test_lowest_code_is_a_value_without_fill(dev, name):
    """no fill declared: -32768 is an ordinary code (the lowest value for s > 0, the highest for s < 0)"""
    doy = _daily(1991, 2020)
    codes = _gen(doy.shape[0], 40, 500, fillfrac=0.0)
    rng = np.random.default_rng(501)
    codes[rng.random(codes.shape) < 0.01] = -32768
    codes[:, 2] = -32768                                             # every sample the lowest code
    codes[rng.random(doy.shape[0]) < 0.3, 3] = -32768
    recipe = RECIPES[name][:2] + (None,) + RECIPES[name][3:]
    for q, negate in ((0.9, False), (0.1, False), (0.0, True), (1.0, True), (0.99, False)):
        th, se = _launch(dev, codes, doy, q, negate, recipe)
        _check(dev, codes, doy, q, negate, recipe, th, se, f"{name} q={q} negate={negate}")
        assert np.isfinite(th).all() and np.isfinite(se).all()


@pytest.fixture(scope="module")
def edge_data():
    doy = _daily(1982, 2021)
    T, C = doy.shape[0], 40
    codes = _gen(T, C, 600)
    t1 = int(np.nonzero(doy == 200)[0][17])
    one = codes[t1, 2]
    codes[:, 2] = FILL                                               # one valid sample: the pools around doy 200
    codes[t1, 2] = one
    codes[(doy >= 95) & (doy <= 105), 3] = FILL                      # pool 100 empty, the cell valid elsewhere
    for c in (4, 34):                                                # (both waves)
        codes[:, c] = 731                                            # constant: every key ties
        codes[:, c + 1] = np.where(np.arange(T) % 3 == 0, -12, 40)  # two values
    codes[np.arange(T) % 5 == 0, 6] = FILL
    return doy, codes, doy[t1]


@pytest.mark.parametrize("name", list(RECIPES))
def test_edge_cells(dev, edge_data, name):
    """a pool with exactly one valid sample, a pool all fill in a cell valid elsewhere (NaN there only), a constant
    cell and a two-valued cell (ties), every recipe, quantiles at both ends and mirrored"""
    doy, codes, d1 = edge_data
    recipe = RECIPES[name]
    for q, negate in ((0.0, False), (0.1, True), (0.15, False), (0.9, True), (0.99, False), (1.0, True)):
        th, se = _launch(dev, codes, doy, q, negate, recipe)
        _check(dev, codes, doy, q, negate, recipe, th, se, f"{name} q={q} negate={negate}")
        if recipe[2] is not None:
            near = np.abs(np.arange(1, 367) - d1) <= 5
            npt.assert_array_equal(np.isfinite(th[:, 2]), near)
            npt.assert_array_equal(np.isnan(th[:, 3]), np.arange(1, 367) == 100)
            x1 = _decoded(codes[:, 2:3], recipe)
            v = x1[np.isfinite(x1)][0]
            npt.assert_array_equal(th[near, 2], -v if negate else v)


@pytest.mark.parametrize("name", ["f64_neg", "fill_only", "f32_pos"])
def test_pitched_input_and_output(dev, name):
    """ld > C and ldo > C: the kernel reads C columns of every row of the codes and writes C columns of every output
    row; the columns behind C keep the sentinel"""
    doy = _daily(1991, 2020)
    C, ld, ldo = 43, 50, 47
    codes = _gen(doy.shape[0], C, 700)
    recipe = RECIPES[name]
    sentinel = -7.125e300
    for q, negate in ((0.9, False), (0.1, True)):
        th, se = _launch(dev, codes, doy, q, negate, recipe, ld=ld, ldo=ldo, sentinel=sentinel)
        assert (th[:, C:] == sentinel).all() and (se[:, C:] == sentinel).all()
        _check(dev, codes, doy, q, negate, recipe, th[:, :C], se[:, :C], f"{name} q={q} negate={negate}")


# ---- 6. seeded random sweep ---------------------------------------------------------------------------------------

def test_seeded_random_recipes_against_the_oracle(dev):
    """30 draws of tools/fuzz_ring2.py's plan / data generator (records of 9..48 tracks, partial years, quantised values,
    NaN shares, infinities, constant cells, cold spells) encoded by its random_packed_recipe() (every recipe, fill codes
    -32768, -999, 0, 32767, both byte orders), percentiles >= 85 or <= 15, against the oracle"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import fuzz_ring2 as fz
    from xmhw_amd.exception import XmhwException
    rng = np.random.default_rng(811)
    done = 0
    seen = set()
    while done < 30:
        x, doy, pct, _, cold, _ = fz.random_ring2_case(rng, (9, 49))
        if 15 < pct < 85:
            continue
        r = fz.random_packed_recipe(rng)
        codes = fz.encode_packed(x, r)
        kw = fz.packed_call_args(r)
        mode = 3 if kw["scale_factor"] is None else (1 if r["decoded"] == "float32" else 2)
        recipe = (kw["scale_factor"], kw["add_offset"], r["fill"], r["decoded"], mode)
        try:
            th, se = _launch(dev, codes, doy, pct / 100.0, cold, recipe, big_endian=r["big_endian"])
        except XmhwException as e:            # (a plan of another kernel: a short tstep year, say)
            assert "sorted-list kernel" in str(e)
            continue
        _check(dev, codes, doy, pct / 100.0, cold, recipe, th, se, f"draw {done}: T={x.shape[0]} C={x.shape[1]} pct={pct} "
               f"cold={cold} {r}")
        seen.add((mode, r["fill"] is None))
        done += 1
    assert {(1, False), (2, False), (3, False), (3, True)} <= seen, seen
