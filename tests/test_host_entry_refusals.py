"""What every entry answers before its first HIP call does not move (CPU, no GPU): the table of
tools/record_entry_refusals.py -- shape, leading-dimension, cap, 2^31, NULL, label-range, length and itemsize refusals, the
zero-size returns, and for every pair of checks that can both apply which one wins -- replayed against
tests/golden/entry_refusals.json, which was recorded before the bindings got their pointer type and float dispatch and the
stage entries their shared steps.  The replay runs in a child process that sees no device and makes sure of that first."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_entry_refusals",
                                                  os.path.join(ROOT, "tools", "record_entry_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def replayed():
    rec = _recorder()
    with open(rec.FIXTURE) as f:
        want = json.load(f)["cases"]
    return rec, rec.run_cases(), want


def test_every_case_answers_as_recorded(replayed):
    rec, got, want = replayed
    h = rec.module()
    table = [case for entry in rec.table(h) for case, _ in entry.calls()]
    assert len(set(table)) == len(table)
    assert sorted(want) == sorted(table)                 # the fixture holds exactly the table's cases ...
    assert sorted(got) == sorted(table)                  # ... and the replay ran every one of them
    moved = {k: (got[k], want[k]) for k in table if got[k] != want[k]}
    assert not moved, "\n".join(f"{k}: {g!r} for {w!r}" for k, (g, w) in moved.items())


def test_no_case_reaches_the_runtime(replayed):
    rec, got, want = replayed
    for outcomes in (got, want):
        assert not [k for k, v in outcomes.items() if rec.reached_the_runtime(v)]


def test_no_binding_with_a_device_pointer_is_left_out(replayed):
    rec = replayed[0]
    h = rec.module()
    rec.covered(h, rec.table(h))
