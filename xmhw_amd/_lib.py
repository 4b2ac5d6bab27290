"""Loader of the HIP extension.  There is NO CPU fallback: if the gfx950
library or its pybind11 module is missing the product path fails loudly."""
import importlib
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_loaded = {}


class HipExtensionMissing(ImportError):
    pass


def _extension(name):
    """The pybind11 module ``xmhw_amd.<name>`` behind the out-of-memory retry, loaded once, or raise.  A module of stage
    bindings ("Entry layer") raises the exception classes of ``_xmhw_hip``, which is loaded first."""
    if name not in _loaded:
        if name != "_xmhw_hip":
            hip()
        try:
            _loaded[name] = _RetryOnNoMem(importlib.import_module(f"xmhw_amd.{name}"))
        except ImportError as e:  # pragma: no cover - build problem
            raise HipExtensionMissing(f"cannot import xmhw_amd.{name}: {e}") from e
    return _loaded[name]


def hip():
    """Return the pybind11 module ``xmhw_amd._xmhw_hip`` or raise."""
    if "_xmhw_hip" not in _loaded and not os.path.exists(os.path.join(_HERE, "libxmhw_amd.so")):
        raise HipExtensionMissing(
            "xmhw_amd/libxmhw_amd.so not found: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C xmhw_amd/csrc`")
    return _extension("_xmhw_hip")


def hip_stress():
    """the bindings of heat_stress()"""
    return _extension("_xmhw_hip_stress")


def hip_regress():
    """the bindings of index_regression()"""
    return _extension("_xmhw_hip_regress")


def hip_composite():
    """the bindings of mhw_composite()"""
    return _extension("_xmhw_hip_composite")


def hip_lagcorr():
    """the bindings of lag_correlation()"""
    return _extension("_xmhw_hip_lagcorr")


def hip_distribution():
    """the bindings of anomaly_distribution()"""
    return _extension("_xmhw_hip_distribution")


def hip_spatialcorr():
    """the bindings of spatial_correlation()"""
    return _extension("_xmhw_hip_spatialcorr")


def hip_coarsen():
    """the bindings of coarsen()"""
    return _extension("_xmhw_hip_coarsen")


def hip_regrid():
    """the bindings of regrid()"""
    return _extension("_xmhw_hip_regrid")


class _RetryOnNoMem:
    """The pybind11 module with one behaviour added: a call that runs out of device memory
    (XMHW_ERR_NOMEM -> MemoryError) is repeated once after the cached large device buffers of
    xmhw_amd.device have been returned to the driver -- allocations made inside the C ABI (plan
    tables, scratch rows, the float32 threshold copy) cannot see that cache otherwise."""

    def __init__(self, mod):
        self._mod = mod
        self._wrapped = {}

    def __getattr__(self, name):
        w = self._wrapped.get(name)
        if w is not None:
            return w
        attr = getattr(self._mod, name)
        if not callable(attr) or isinstance(attr, type):
            return attr

        def call(*args, **kw):
            try:
                return attr(*args, **kw)
            except MemoryError:
                from .device import release_device_cache
                if not release_device_cache():
                    raise
                return attr(*args, **kw)

        call.__name__ = name
        self._wrapped[name] = call
        return call


def require_gpu():
    """Raise unless a HIP device is usable."""
    h = hip()
    n = h.device_count()          # raises HipError without a device/driver
    if n < 1:
        raise h.HipError("no HIP device visible")
    return n
