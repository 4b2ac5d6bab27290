"""The Python-visible surface of _xmhw_hip does not move (CPU, no GPU): every public name, the argument names, order and
defaults of every callable, the constants and the exception bases equal tests/golden/binding_signatures.json, recorded by
tools/record_binding_signatures.py before the bindings got their pointer argument type -- and the generated annotations
too, where the installed pybind11 is the one the fixture was recorded with.  The bindings listed in DELETED had no user
and are gone; nothing else is."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (a fixture recorded anew no longer holds these names: the list is emptied with it)
DELETED = ("clim_dev", "memcpy_d2h_bytes", "stream_destroy", "memcpy_d2h_async", "memcpy2d_h2d_async",
           "comm_allgather_i64_begin", "comm_allgather_i64_end", "plan_set_ring2", "plan_ring2_in_use")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_binding_signatures",
                                                  os.path.join(ROOT, "tools", "record_binding_signatures.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


@pytest.fixture(scope="module")
def surfaces():
    rec = _recorder()
    with open(rec.FIXTURE) as f:
        want = json.load(f)
    return rec, rec.surface(rec.module()), want


def test_names_are_the_recorded_ones_minus_the_deleted(surfaces):
    rec, got, want = surfaces
    assert set(DELETED) <= set(want["names"])
    assert not set(DELETED) & set(got)
    assert sorted(got) == sorted(set(want["names"]) - set(DELETED))


def test_arguments_constants_and_bases_are_equal(surfaces):
    rec, got, want = surfaces
    same_pybind11 = rec.pybind11_version() == want["pybind11"]
    n = 0
    for name, now in got.items():
        then = want["names"][name]
        if "signature" not in then:
            assert now == then, name
            continue
        assert rec.arguments(now["signature"]) == rec.arguments(then["signature"]), name
        if same_pybind11:
            assert now["signature"] == then["signature"], name
        n += 1
    assert n > 100          # the parse found the callables


def test_argument_parser():
    rec = _recorder()
    sig = "f(a: int, b: numpy.ndarray[numpy.int32], c: float = 0.0, stream: int = 0) -> None"
    assert rec.arguments(sig) == [("a", None), ("b", None), ("c", "0.0"), ("stream", "0")]
    assert rec.arguments("g() -> int") == []
