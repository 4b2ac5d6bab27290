"""The four row-walking stages of the object chain called raw, as the C ABI takes them: xmhw_object_tracks, _parts,
_genealogy and _shape on the arguments of their *_device() functions with nothing checked on the way, and those
arguments captured from the public functions.  TEST INFRASTRUCTURE ONLY (GPU tests)."""
import numpy as np

import track_genealogy_oracle as go
import track_parts_oracle as po
import track_shape_oracle as so
import tracks_oracle as to

I32, I64 = np.int32, np.int64
# the dtypes of the arguments of tracks_device(), track_parts_device(), track_genealogy_device(), track_shape_device()
DTYPES = dict(tracks=(I32, I32, I32, I32, I64, I32, I64), parts=(I32, I32, I32, I32, I64, I32, I64, I64, I32, I64),
              genealogy=(I32, I32, I32, I32, I64, I32, I64, I32, I64), shape=(I32, I32, I32, I32, I64, I32, I64, I32, I64))
CLASSES = ("open", "coast", "border")


def _upload(s, stage, args):
    args = [np.ascontiguousarray(a, dtype=t) for a, t in zip(args, DTYPES[stage])]
    return args, [s.upload(a).ptr for a in args]


def _bad(d_bad):
    return int(d_bad.to_array((1,), np.int32)[0])


def raw_tracks(args):
    """(dict of n_cells (L,) and sums (4, L), n_bad)"""
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceScope
    with DeviceScope() as s:
        (start, _, _, _, vec, time_start, offsets), d = _upload(s, "tracks", args)
        n, C, m, L = start.shape[0], vec.shape[1], time_start.shape[0], int(offsets[-1])
        d_cnt, d_sums, d_bad = s.alloc(4 * (L + 1)), s.alloc(32 * (L + 1)), s.alloc(4)
        hip().object_tracks(d[0], d[1], n, d[2], d[3], C, d[4], C, d[5], d[6], m, L, d_cnt.ptr, d_sums.ptr, L + 1, d_bad.ptr)
        hip().stream_sync(0)
        return dict(n_cells=d_cnt.to_array((L + 1,), I32)[:L], sums=d_sums.to_array((4, L + 1), I64)[:, :L]), _bad(d_bad)


def raw_parts(args):
    """(dict of the three arrays, n_bad)"""
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceScope
    with DeviceScope() as s:
        (start, _, _, _, _, nbr, wq, vox_off, time_start, offsets), d = _upload(s, "parts", args)
        n, C, m, L, V = start.shape[0], wq.shape[0], time_start.shape[0], int(offsets[-1]), int(vox_off[-1])
        d_np, d_cl, d_al, d_bad = s.alloc(4 * L), s.alloc(4 * L), s.alloc(8 * L), s.alloc(4)
        hip().object_parts(d[0], d[1], d[2], d[3], n, d[4], C, d[5], nbr.shape[1], d[6], d[7], V, d[8], d[9], m, L, d_np.ptr,
                           d_cl.ptr, d_al.ptr, d_bad.ptr)
        hip().stream_sync(0)
        return dict(n_parts=d_np.to_array((L,), I32), cells_largest=d_cl.to_array((L,), I32),
                    area_largest_q=d_al.to_array((L,), I64)), _bad(d_bad)


def raw_genealogy(args):
    """(dict of the six counts and the four sorted edge arrays, n_bad); the set never overflows: its capacity is that of
    track_genealogy_device()"""
    from xmhw_amd import track_genealogy as tg
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceScope
    with DeviceScope() as s:
        (start, end, slot, cell, row_offsets, nbr, vox_off, time_start, offsets), d = _upload(s, "genealogy", args)
        n, C, m, L, V = start.shape[0], row_offsets.shape[0] - 1, time_start.shape[0], int(offsets[-1]), int(vox_off[-1])
        cap, F = tg.edge_capacity(start, end, slot, cell), len(tg.COUNT_FIELDS)
        d_counts, d_edges, d_ne, d_bad, d_over = s.alloc(4 * F * L), s.alloc(8 * max(cap, 1)), s.alloc(8), s.alloc(4), s.alloc(4)
        hip().object_genealogy(d[0], d[1], d[2], d[3], n, d[4], C, d[5], nbr.shape[1], d[6], V, d[7], d[8], m, L, d_counts.ptr,
                               d_edges.ptr, cap, d_ne.ptr, d_bad.ptr, d_over.ptr)
        hip().stream_sync(0)
        E = int(d_ne.to_array((1,), I64)[0])
        assert 0 <= E <= cap and int(d_over.to_array((1,), I32)[0]) == 0
        counts = d_counts.to_array((F, L), I32)
        keys = d_edges.to_array((max(cap, 1),), np.uint64)[:E]
        out = {k: counts[i] for i, k in enumerate(tg.COUNT_FIELDS)}
        out.update(zip(tg.EDGE_FIELDS, tg.edges_of_keys(keys, start, slot, cell, vox_off)))
        return out, _bad(d_bad)


def raw_shape(args):
    """(dict of the seven arrays, n_bad)"""
    from xmhw_amd._lib import hip
    from xmhw_amd.device import DeviceScope
    with DeviceScope() as s:
        (start, _, _, _, _, faces, _, time_start, offsets), d = _upload(s, "shape", args)
        n, C, m, L = start.shape[0], faces.shape[0], time_start.shape[0], int(offsets[-1])
        d_edges, d_perim, d_cells, d_bad = s.alloc(12 * L), s.alloc(24 * L), s.alloc(4 * L), s.alloc(4)
        hip().object_shape(d[0], d[1], d[2], d[3], n, d[4], C, d[5], 4, d[6], d[7], d[8], m, L, d_edges.ptr, d_perim.ptr,
                           d_cells.ptr, d_bad.ptr)
        hip().stream_sync(0)
        edges, perim = d_edges.to_array((3, L), I32), d_perim.to_array((3, L), I64)
        out = {f"edges_{c}": edges[k] for k, c in enumerate(CLASSES)}
        out.update({f"perimeter_{c}_q": perim[k] for k, c in enumerate(CLASSES)})
        out["cells_edge"] = d_cells.to_array((L,), I32)
        return out, _bad(d_bad)


RAW = dict(tracks=raw_tracks, parts=raw_parts, genealogy=raw_genealogy, shape=raw_shape)


def oracle_for(stage, ds, obj):
    """the stage oracle of ``stage`` on the grid of ``ds``: a stand-in for its *_device()"""
    return to.stage_voxels if stage == "tracks" else dict(parts=po, genealogy=go, shape=so)[stage].stage_for(ds, obj)


def captured_arguments(stage, ds, obj, **kw):
    """the arguments the public function of ``stage`` hands to its device stage, as arrays of their own"""
    import xmhw_amd
    public = dict(tracks=xmhw_amd.mhw_tracks, parts=xmhw_amd.mhw_track_parts, genealogy=xmhw_amd.mhw_track_genealogy,
                  shape=xmhw_amd.mhw_track_shape)[stage]
    oracle, seen = oracle_for(stage, ds, obj), {}

    def compute(*args):
        seen["args"] = args
        return oracle(*args)

    public(ds, obj, _compute=compute, **kw)
    return [np.array(a) for a in seen["args"]]
