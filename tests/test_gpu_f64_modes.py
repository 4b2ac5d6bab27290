"""Every dispatchable instantiation of the ring kernels' 64-bit mode on clustered doubles (tests/f64_mode_cases.py), at the
fewest and at the most tracks that dispatch to it, against the float64 oracle.

The 64-bit mode selects on the high word of a 64-bit key and settles ties on the low word.  The samples here are
distinct doubles that share the high word of their level, positive and negative (a negative double's low words order the
other way round), with exact repeats, a cell near -1.8, +-0, +-inf, NaN and doubles outside float32's range: on more than
half of the rows the quantile's bracket can only be told apart by the low words (tests/test_f64_mode_cases.py checks
that of the inputs).  The "most" records start and end inside a year, so the first and last tracks are partial and the
held Feb-29 step rotates both rings; they run negated at q = 0.1 in three chunks.

The switches that move the float64 route are read once per process: the default leg runs here, every other leg
(XMHW_RING3_F64=0 -- the second-generation 8-lane kernels, which nothing else runs on a GPU; XMHW_RING3_F64_LANES=8 -- the
third-generation 8-lane kernel with full lanes at 2 tracks per lane; XMHW_RING3_F64=0 with XMHW_RING2_F64_LDS=0) in
one child process (tests/f64_mode_child.py), one at a time.  A child that fails, dies or runs out of time fails its
leg's tests with its output, and no later leg is started.

Per case: the launch (narrowing off) and the gated launch (narrowing on) are the expected instantiation; narrowed() is
False; thresh equals oracle_fast.raw_clim bit for bit (exact selection + numpy's lerp in float64), NaN positions
included; seas to rtol = atol = 1e-12 (float64 sums in another order: tests/test_gpu_parity_f64.py); narrowing on and off
agree bit for bit; the padding columns of a pitched output still hold their 0xFF bytes."""
import json
import subprocess
import sys

import numpy as np
import numpy.testing as npt
import pytest

import oracle_fast as fast
import f64_mode_cases as fc
import f64_mode_child as child
from test_f64_mode_cases import CHILD, child_env

pytestmark = pytest.mark.gpu

# The default leg in this process on an MI355X, data generation and oracle included: 4.3 s for its 25 cases (the
# longest leg: it has the most cases and the longest records).  A child gets five times that, scaled by its case
# count, plus 60 s for interpreter start and device initialisation; one that needs longer counts as hung unless its
# log shows cases still completing.
DEFAULT_LEG_SECONDS = 4.3
DEFAULT_LEG_CASES = 25
assert len(fc.CASES[0]) == DEFAULT_LEG_CASES


def child_time_limit(leg):
    return 5.0 * DEFAULT_LEG_SECONDS * len(fc.CASES[leg]) / DEFAULT_LEG_CASES + 60.0


@pytest.fixture(scope="module")
def dev():
    from xmhw_amd._lib import require_gpu
    require_gpu()
    import xmhw_amd.device as d
    return d


_broken = []                   # the first leg whose child failed: no later child is started


def _start(leg, tmp):
    if _broken:
        pytest.fail(f"leg {leg} not started: the child of leg {_broken[0]} failed")
    out = tmp / f"leg{leg}.npz"
    limit = child_time_limit(leg)
    try:
        p = subprocess.run([sys.executable, CHILD, str(leg), str(out)], env=child_env(leg), timeout=limit,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _broken.append(leg)
        log = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"leg {leg} {fc.LEGS[leg]}: the child was still running after {limit:.0f} s\n{log[-4000:]}")
    if p.returncode != 0:
        _broken.append(leg)
        how = f"signal {-p.returncode}" if p.returncode < 0 else f"status {p.returncode}"
        pytest.fail(f"leg {leg} {fc.LEGS[leg]}: the child ended with {how}\n{p.stdout[-4000:]}")
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    """leg -> what its child wrote; a child is started when the first test of its leg asks for it (the tests run in
    the order of the legs), never two at a time"""
    from xmhw_amd._lib import require_gpu
    require_gpu()
    tmp = tmp_path_factory.mktemp("f64_modes")
    done = {}

    def get(leg):
        if leg not in done:
            try:
                done[leg] = _start(leg, tmp)
            except BaseException as e:
                done[leg] = e
        if isinstance(done[leg], BaseException):
            raise done[leg]
        return done[leg]

    return get


def _same(a, b, msg):
    """bit for bit in the sense of the parity tests: equal values, NaN where NaN"""
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64, msg
    if not np.array_equal(a, b, equal_nan=True):
        npt.assert_array_equal(a, b, err_msg=msg)


def _check(case, got):
    cid = case["id"]
    expect = list(case["expect"])
    off, on = got["route"]["off"], got["route"]["on"]
    assert len(off) == 1 and off[0][:4] == expect and off[0][4:] == [0, 0], (cid, off)
    assert len(on) == 2 and on[0][4:] == [1, 0] and on[1][:4] == expect and on[1][4:] == [0, 1], (cid, on)
    assert bool(got["narrowed"]) is False, cid
    doy, x = fc.samples(case)
    with np.errstate(invalid="ignore"):
        doys, th0, se0 = fast.raw_clim(-x if case["negate"] else x, doy, case["q"], fc.W)
    D = doys.shape[0]
    ldo = fc.PITCH["ldo"] if case["pitched"] else fc.C
    for tag in ("off", "on"):
        th, se = got["th_" + tag], got["se_" + tag]
        assert th.shape == se.shape == (D, ldo), (cid, tag, th.shape)
        _same(th[:, :fc.C], th0, f"{cid}: thresh, narrowing {tag}, against the oracle")
        with np.errstate(invalid="ignore"):
            npt.assert_allclose(se[:, :fc.C], se0, rtol=1e-12, atol=1e-12, equal_nan=True,
                                err_msg=f"{cid}: seas, narrowing {tag}, against the oracle")
        if case["pitched"]:
            sentinel = np.full((D, ldo - fc.C), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            for out in (th, se):
                npt.assert_array_equal(np.ascontiguousarray(out[:, fc.C:]).view(np.uint64), sentinel,
                                       err_msg=f"{cid}: padding columns, narrowing {tag}")
    _same(got["th_on"][:, :fc.C], got["th_off"][:, :fc.C], f"{cid}: thresh, narrowing on against off")
    _same(got["se_on"][:, :fc.C], got["se_off"][:, :fc.C], f"{cid}: seas, narrowing on against off")
    # the all-NaN cell is NaN, the clustered cells are not
    assert np.isnan(got["th_off"][:, fc.ALL_NAN]).all() and not np.isnan(got["th_off"][:, [0, fc.C - 1]]).any(), cid


@pytest.mark.parametrize("no", range(len(fc.CASES[0])), ids=[c["id"] for c in fc.CASES[0]])
def test_default_leg(dev, no):
    _check(fc.CASES[0][no], child.run_case(dev, fc.CASES[0][no]))


def _from_child(saved, no):
    got = {k: saved[f"{no}_{k}"] for k in ("th_off", "se_off", "th_on", "se_on", "narrowed")}
    got["route"] = json.loads(str(saved[f"{no}_route"]))
    return got


@pytest.mark.parametrize("no", range(len(fc.CASES[1])), ids=[c["id"] for c in fc.CASES[1]])
def test_second_generation_8_lane_leg(legs, no):
    """XMHW_RING3_F64=0: the XMHW_R2N / XMHW_R2L entries of variant 8, 2 .. 6 tracks per lane"""
    _check(fc.CASES[1][no], _from_child(legs(1), no))


@pytest.mark.parametrize("no", range(len(fc.CASES[2])), ids=[c["id"] for c in fc.CASES[2]])
def test_third_generation_8_lane_leg(legs, no):
    """XMHW_RING3_F64_LANES=8: the third-generation 8-lane kernel on 13 .. 20 tracks"""
    _check(fc.CASES[2][no], _from_child(legs(2), no))


@pytest.mark.parametrize("no", range(len(fc.CASES[3])), ids=[c["id"] for c in fc.CASES[3]])
def test_16_lane_leg_at_3_tracks_per_lane(legs, no):
    """XMHW_RING3_F64=0 with XMHW_RING2_F64_LDS=0: 33 .. 48 tracks on the 16-lane layout"""
    _check(fc.CASES[3][no], _from_child(legs(3), no))
