"""Which chunks the sorted-list kernel settles directly (csrc/plan.cpp: SortedPlan::direct; C ABI
xmhw_plan_sorted_direct), on the CPU: the one-row chunk of Feb 29 of every daily record with a leap year, nothing on a
calendar without one, nothing with XMHW_SORTED_ONEROW=0 -- a process-wide switch read once, so both settings are asked
in fresh child processes -- and the chunks, table rows, flags, kernel facts and the route are the same either way."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sorted_onerow_cases as soc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _child(tmp_path, switch):
    out = tmp_path / f"host_{switch}.npz"
    env = dict(os.environ)
    env.pop("XMHW_SORTED_ONEROW", None)
    if switch is not None:
        env["XMHW_SORTED_ONEROW"] = switch
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sorted_onerow_cases.py"), ROOT, "host", str(out)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    with np.load(out) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("onerow_host")
    return {"default": _child(tmp, None), "on": _child(tmp, "1"), "off": _child(tmp, "0")}


LEAP = [name for name, _, _ in soc.RECORDS] + [f"{y}y_from_1980" for y in soc.HOST_YEARS]


@pytest.mark.parametrize("name", LEAP)
def test_daily_records_with_a_leap_year_have_one_direct_chunk(answers, name):
    for setting in ("default", "on"):
        np.testing.assert_array_equal(answers[setting][f"direct_{name}"], 1)
    # ... and it is the row of doy 60: one output row, pooled by the leap years alone
    chunks = answers["on"][f"chunks_{name}"]
    one = [(int(b), int(e)) for _, b, e, _ in chunks if e - b == 1]
    assert one == [(59, 60)], one


@pytest.mark.parametrize("name", ["noleap_daily", "noleap_6hourly"])
def test_no_leap_year_no_direct_chunk(answers, name):
    for setting in ("default", "on", "off"):
        np.testing.assert_array_equal(answers[setting][f"direct_{name}"], 0)


def test_the_switch_turns_every_direct_chunk_off(answers):
    for name in LEAP:
        np.testing.assert_array_equal(answers["off"][f"direct_{name}"], 0)


def test_plan_table_info_and_route_do_not_depend_on_the_switch(answers):
    on, off = answers["on"], answers["off"]
    assert sorted(on) == sorted(off)
    n = 0
    for k in on:
        if k.startswith("direct_"):
            continue
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
        n += 1
    assert n == 5 * (len(LEAP) + 2)
