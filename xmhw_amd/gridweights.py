"""Cell weights on the spatial grid, shared by mhw_coverage(), mhw_objects() and mhw_tracks(): the ``weights``
argument (None, "coslat" or an array) as float64 (N,) in stacked order, and its fixed-point quantisation."""
import numpy as np

from .exception import XmhwException

LAT_NAMES = ("lat", "latitude", "y", "yt_ocean", "nav_lat")
LON_NAMES = ("lon", "longitude", "x", "xt_ocean", "nav_lon")


def quantise_weights(w, bits=31):
    """(wq int64, weight_unit): wq = rint(w / w.max() * 2**bits); w finite, >= 0, not all zero."""
    w = np.asarray(w, dtype=np.float64)
    if w.size == 0 or not np.isfinite(w).all():
        raise XmhwException("weights should be finite numbers")
    if (w < 0).any():
        raise XmhwException("weights should be >= 0")
    wmax = float(w.max())
    if not wmax > 0:
        raise XmhwException("weights are all zero")
    one = 1 << int(bits)
    return np.rint(w / wmax * one).astype(np.int64), wmax / one


def on_grid(a, what, dims, tdim, sdims, sshape):
    """An array given on the spatial grid (the non-time dims in the order of `temp`) -> (N,) in stacked order."""
    a = np.asarray(a)
    rest = [d for d in dims if d != tdim]
    shape = tuple(sshape[sdims.index(d)] for d in rest)
    if a.shape != shape:
        raise XmhwException(f"{what} should have the shape of the spatial grid {dict(zip(rest, shape))}, got {a.shape}")
    return np.transpose(a, [rest.index(d) for d in sdims]).reshape(-1)


def coslat(coords, sdims, sshape):
    name = next((d for d in sdims if d.lower() in LAT_NAMES), None)
    if name is None:
        raise XmhwException(f"weights='coslat' needs a latitude dimension (lat / latitude), got {sdims}")
    w = np.cos(np.deg2rad(np.asarray(coords[name], dtype=np.float64)))
    w = np.where(np.abs(w) < 1e-15, 0.0, w)                     # cos(90 degrees) is 6e-17 in float64
    shape = [1] * len(sdims)
    shape[sdims.index(name)] = -1
    return np.broadcast_to(w.reshape(shape), sshape).reshape(-1)


def resolve_weights(weights, coords, dims, tdim, sdims, sshape, point=False):
    """The ``weights`` argument as float64 (N,) in stacked order (N = 1 for a single-point series).  ``dims``: the
    dims an array of weights is given on once ``tdim`` is taken out (the order of `temp`, or ``sdims`` itself)."""
    N = 1 if point else int(np.prod(sshape, dtype=np.int64))
    if weights is None:
        return np.ones(N)
    if isinstance(weights, str):
        if weights != "coslat":
            raise XmhwException(f"weights should be None, 'coslat' or an array, got {weights!r}")
        return np.ones(1) if point else coslat(coords, sdims, sshape)
    w = np.asarray(weights, dtype=np.float64).reshape(-1) if point else \
        on_grid(np.asarray(weights, dtype=np.float64), "weights", dims, tdim, sdims, sshape)
    if w.shape != (N,):
        raise XmhwException("weights should have one entry per cell")
    return w


def weights_label(weights):
    """what the result's ``attrs["weights"]`` says"""
    return "coslat" if isinstance(weights, str) else ("uniform" if weights is None else "array")
