"""The threshold dispatch does not move (CPU, no GPU): the sweep of tools/record_routes.py -- 8 windows x 1..200 tracks x
9 layouts x 3 kernel selectors x narrowing on / off x float32 / float64 x 5 quantiles, the chunk and piece counts of six
daily calendars, and each environment switch in a process of its own -- replayed against tests/golden/threshold_routes.npz,
which was recorded from the dispatch as it stood before xmhw_plan_route became its only source.  Every record must be
equal: the route, xmhw_plan_layout_in_use, xmhw_plan_f64_mode, the kernel of xmhw_plan_info, xmhw_plan_chunks_in_use and
the pieces of xmhw_plan_sorted_info."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_routes", os.path.join(ROOT, "tools", "record_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def replayed():
    rec = _recorder()
    return rec, rec.flatten(rec.run_legs())


def test_routes_equal_the_recorded_dispatch(replayed):
    rec, got = replayed
    with np.load(rec.FIXTURE) as z:
        want = {k: z[k] for k in z.files}
    assert tuple(want.pop("legs")) == rec.LEGS
    assert sorted(got) == sorted(want)
    full = (len(rec.WINDOWS), len(rec.TRACKS), len(rec.LAYOUTS), len(rec.KERNELS), 2, len(rec.ELEM_BYTES),
            len(rec.QUANTILES), rec.ROUTE_WORDS)
    for i, leg in enumerate(rec.LEGS):
        # no case left out: the whole sweep in the default leg, the whole w = 5 slice in the others
        assert want[f"{i}_routes"].shape == (full if i == 0 else (1,) + full[1:]), leg
        assert want[f"{i}_counts"].shape == (len(rec.YEARS), len(rec.LAYOUTS), len(rec.CHUNKS), len(rec.CELLS), 4), leg
    for k in sorted(want):
        leg = rec.LEGS[int(k.split("_")[0])]
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (leg, k)
        bad = np.argwhere(got[k] != want[k])
        assert bad.shape[0] == 0, (f"{leg}: {k} differs in {bad.shape[0]} values, first at {tuple(bad[0])}: "
                                   f"{got[k][tuple(bad[0])]} for {want[k][tuple(bad[0])]}")


def test_sweep_reaches_every_family_and_sequence(replayed):
    """the fixture is only a pin if the sweep exercises the dispatch: all five launch sequences and every family occur"""
    rec, got = replayed
    r = got["0_routes"].reshape(-1, rec.ROUTE_WORDS)
    r = r[r[:, 1] > 0]
    fam0, fam1, narrows0, gated1 = r[:, 2], r[:, 9], r[:, 6], r[:, 14]
    assert set(np.unique(fam0)) == {0, 1, 2, 3, 5}              # generic, ring1, ring2, ring3, sorted first
    one, two = r[:, 1] == 1, r[:, 1] == 2
    assert (one & (fam0 == 5)).any() and (one & (fam0 == 0)).any() and (one & np.isin(fam0, (1, 2, 3))).any()
    assert (two & (narrows0 == 1) & (gated1 == 1) & np.isin(fam1, (2, 3))).any()
    assert (two & (narrows0 == 1) & (gated1 == 1) & (fam1 == 0)).any()
    assert (got["0_routes"][..., 0] == 3).any() and (got["0_refused"] == 3).any()          # refused calls and layouts
    for i in range(1, len(rec.LEGS)):
        # (XMHW_RING2_F64_LDS=0 moves nothing on its own: the third-generation 64-bit mode serves those records first)
        moved = (got[f"{i}_routes"] != got["0_routes"][rec.WINDOWS.index(5)][None]).any()
        assert moved == (rec.LEGS[i] != "XMHW_RING2_F64_LDS=0"), rec.LEGS[i]
