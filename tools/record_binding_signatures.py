"""The Python-visible surface of _xmhw_hip: for every public name the signature line pybind11 generated (callables), the
value (constants) or the base class (exceptions), and the pybind11 version that generated them.  No GPU.

    python tools/record_binding_signatures.py      writes tests/golden/binding_signatures.json

tests/test_host_binding_signatures.py compares the built module against it."""
import importlib
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "binding_signatures.json")


def module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("xmhw_amd._xmhw_hip")


def surface(h):
    out = {}
    for name in sorted(n for n in dir(h) if not n.startswith("_")):
        obj = getattr(h, name)
        if isinstance(obj, type):
            out[name] = {"exception": obj.__base__.__name__}
        elif callable(obj):
            out[name] = {"signature": obj.__doc__.splitlines()[0]}
        else:
            out[name] = {"constant": obj}
    return out


def arguments(signature):
    """'f(a: int, b: numpy.ndarray[numpy.int32], c: int = 0) -> None' -> [('a', None), ('b', None), ('c', '0')]"""
    inner = signature[signature.index("(") + 1:signature.rindex(") ->")]
    parts, depth, cur = [], 0, ""
    for ch in inner:
        depth += ch in "[("
        depth -= ch in "])"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur)
    out = []
    for p in parts:
        name, _, rest = p.strip().partition(":")
        out.append((name.strip(), rest.rpartition(" = ")[2].strip() if " = " in rest else None))
    return out


def pybind11_version():
    import pybind11
    return pybind11.__version__


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump({"pybind11": pybind11_version(), "names": surface(module())}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")
