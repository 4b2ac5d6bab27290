"""The two context managers of the host layer (xmhw_amd/device.py) without a device: DeviceScope on stand-in
buffers (a zero-byte DeviceBuffer allocates nothing), as_xmhw_errors on exceptions of the bindings raised by hand."""
import numpy as np
import pytest

from xmhw_amd import XmhwException
from xmhw_amd._lib import hip
from xmhw_amd.device import DeviceBuffer, DeviceScope, as_xmhw_errors


class Fake:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def free(self):
        self.log.append(self.name)


def test_scope_frees_what_it_owns_in_order_and_in_every_case():
    log = []
    with pytest.raises(KeyError):                                  # the scope does not translate exceptions
        with DeviceScope() as s:
            a, b, c = (s.adopt(Fake(k, log)) for k in "abc")
            assert s.adopt(None) is None
            assert s.release(b) is b
            assert s.release(Fake("stranger", log)) is not None    # not owned: handed through
            raise KeyError("x")
    assert log == ["a", "c"]
    s.free()                                                       # nothing is freed twice
    assert log == ["a", "c"]


def test_scope_alloc_and_upload_return_owned_buffers():
    with DeviceScope() as s:
        z = s.alloc(0)
        e = s.upload(np.zeros(0))
        assert isinstance(z, DeviceBuffer) and isinstance(e, DeviceBuffer) and z.ptr == 0 and e.nbytes == 0
        assert s._owned == [z, e]
    assert s._owned == []


def test_error_mapping():
    h = hip()
    assert issubclass(h.Unsupported, h.HipError) and not issubclass(h.InvalidArgument, h.HipError)
    with pytest.raises(XmhwException, match="^bad argument$") as e:
        with as_xmhw_errors():
            raise h.InvalidArgument("bad argument")
    assert isinstance(e.value.__cause__, h.InvalidArgument)
    with pytest.raises(h.Unsupported):                             # not asked for: passes through
        with as_xmhw_errors():
            raise h.Unsupported("too large (code 3)")
    with pytest.raises(XmhwException, match=r"^too large \(code 3\)$"):
        with as_xmhw_errors(also="Unsupported"):
            raise h.Unsupported("too large (code 3)")
    with pytest.raises(XmhwException, match=r"^too large \(code 3\): take fewer$"):
        with as_xmhw_errors(also="Unsupported", hint="take fewer"):
            raise h.Unsupported("too large (code 3)")
    with pytest.raises(XmhwException, match="^bad argument$"):     # the hint belongs to Unsupported alone
        with as_xmhw_errors(also="Unsupported", hint="take fewer"):
            raise h.InvalidArgument("bad argument")
    with pytest.raises(h.HipError):                                # any other HipError passes through ...
        with as_xmhw_errors(also="Unsupported"):
            raise h.HipError("hipErrorLaunchFailure (code 2)")
    with pytest.raises(XmhwException, match="code 2"):             # ... unless the site asks for all of them
        with as_xmhw_errors(also="HipError"):
            raise h.HipError("hipErrorLaunchFailure (code 2)")
    with pytest.raises(MemoryError):
        with as_xmhw_errors(also="HipError"):
            raise MemoryError()
