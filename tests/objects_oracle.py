"""mhw_objects() restated in plain Python / numpy: the definition the device is compared with.

Three routes to the same partition of the table rows:

* objects_graph(): the event graph with a sequential union-find, reductions by a loop over the rows (the
  signature of xmhw_amd.objects.objects_device, so it also serves as its stand-in);
* voxel_roots(): independent of the graph -- the rows are rasterised into a (T, ny, nx) bool volume that is
  flood-filled with an explicit stack, with the neighbourhood written out voxel by voxel (handles `periodic`,
  which scipy.ndimage.label cannot);
* objects_edges(): the graph again, vectorised (edge list from two searchsorted calls per neighbour column,
  components by scipy.sparse.csgraph where scipy imports, min-label propagation otherwise) for the large GPU
  cases.
"""
import numpy as np

PER_OBJECT = ("n_events", "n_cells", "time_start", "time_end", "cell_days", "area_days_q", "intensity_max", "peak_row")


def _cells(offsets):
    offsets = np.asarray(offsets, dtype=np.int64)
    return np.repeat(np.arange(offsets.shape[0] - 1, dtype=np.int64), np.diff(offsets))


def reduce_rows(root, start, end, imax, cell, wq):
    """per object (ascending root): the PER_OBJECT numbers, row by row"""
    roots = sorted(set(int(r) for r in root))
    slot = {r: k for k, r in enumerate(roots)}
    m = len(roots)
    out = dict(n_events=np.zeros(m, np.int32), n_cells=np.zeros(m, np.int32), time_start=np.full(m, 2**31 - 1, np.int32),
               time_end=np.full(m, -1, np.int32), cell_days=np.zeros(m, np.int64), area_days_q=np.zeros(m, np.int64),
               intensity_max=np.full(m, np.nan), peak_row=np.full(m, -1, np.int32))
    seen = [set() for _ in range(m)]
    for r in range(len(root)):
        k = slot[int(root[r])]
        d = int(end[r]) - int(start[r]) + 1
        out["n_events"][k] += 1
        seen[k].add(int(cell[r]))
        out["time_start"][k] = min(out["time_start"][k], start[r])
        out["time_end"][k] = max(out["time_end"][k], end[r])
        out["cell_days"][k] += d
        out["area_days_q"][k] += int(wq[cell[r]]) * d
        v = float(imax[r]) + 0.0                                  # -0.0 counts as 0.0
        if v == v and (out["peak_row"][k] < 0 or v > out["intensity_max"][k]):      # a tie keeps the earlier row
            out["intensity_max"][k], out["peak_row"][k] = v, r
    out["n_cells"][:] = [len(s) for s in seen]
    return out


def objects_graph(start, end, imax, offsets, nbr, gap, wq):
    n = len(start)
    cell = _cells(offsets)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a in range(n):
        for nc in nbr[cell[a]]:
            if nc < 0:
                continue
            for b in range(int(offsets[nc]), int(offsets[nc + 1])):
                if start[a] <= end[b] + gap and start[b] <= end[a] + gap:
                    ra, rb = find(a), find(b)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(x) for x in range(n)], dtype=np.int32)
    return dict(root=root, **reduce_rows(root, start, end, imax, cell, wq))


def rasterise(start, end, flat, sshape, T):
    ny, nx = sshape
    vol = np.zeros((T, ny, nx), dtype=bool)
    for r in range(len(start)):
        vol[start[r]:end[r] + 1, flat[r] // nx, flat[r] % nx] = True
    return vol


def voxel_roots(start, end, flat, sshape, T, connectivity, periodic_axis=None):
    """root (n,): the smallest row of the connected component of voxels that holds the row's voxels"""
    ny, nx = sshape
    vol = rasterise(start, end, flat, sshape, T)
    if connectivity == 6:
        steps = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    else:
        steps = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    label = np.full(vol.shape, -1, dtype=np.int64)
    nlab = 0
    for t0, i0, j0 in zip(*np.nonzero(vol)):
        if label[t0, i0, j0] >= 0:
            continue
        label[t0, i0, j0] = nlab
        stack = [(int(t0), int(i0), int(j0))]
        while stack:
            t, i, j = stack.pop()
            for dt, di, dj in steps:
                tt, ii, jj = t + dt, i + di, j + dj
                if periodic_axis == 0:
                    ii %= ny
                if periodic_axis == 1:
                    jj %= nx
                if not (0 <= tt < T and 0 <= ii < ny and 0 <= jj < nx) or (tt, ii, jj) == (t, i, j):
                    continue
                if vol[tt, ii, jj] and label[tt, ii, jj] < 0:
                    label[tt, ii, jj] = nlab
                    stack.append((tt, ii, jj))
        nlab += 1
    lab = np.array([label[start[r], flat[r] // nx, flat[r] % nx] for r in range(len(start))], dtype=np.int64)
    for r in range(len(start)):                                   # every voxel of a row carries one label
        assert (label[start[r]:end[r] + 1, flat[r] // nx, flat[r] % nx] == lab[r]).all()
    first = np.full(nlab, len(start), dtype=np.int64)
    np.minimum.at(first, lab, np.arange(len(start)))
    return first[lab].astype(np.int32), label


def roots_from_labels(lab):
    """a labelling of the rows -> the smallest row of every row's class"""
    lab = np.asarray(lab, dtype=np.int64)
    first = np.full(int(lab.max()) + 1 if lab.size else 0, lab.shape[0], dtype=np.int64)
    np.minimum.at(first, lab, np.arange(lab.shape[0]))
    return first[lab].astype(np.int32)


def edge_list(start, end, offsets, nbr, gap):
    """(a, b) row pairs of the event graph, every pair once per direction it is seen from"""
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    cell = _cells(offsets)
    M = int(end.max()) + 4 if end.size else 4                     # cell * M + time + 1 is sorted over the whole table
    ekey, skey = cell * M + end + 1, cell * M + start + 1
    rows = np.arange(start.shape[0], dtype=np.int64)
    ea, eb = [], []
    for k in range(nbr.shape[1]):
        nc = nbr[cell, k].astype(np.int64)
        ok = nc >= 0
        lo = np.searchsorted(ekey, nc[ok] * M + start[ok] - gap + 1, side="left")     # the first row with end >= start - gap
        hi = np.searchsorted(skey, nc[ok] * M + end[ok] + gap + 1, side="right")      # past the last with start <= end + gap
        cnt = hi - lo
        assert (cnt >= 0).all()
        a = np.repeat(rows[ok], cnt)
        first = np.repeat(lo, cnt)
        within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ea.append(a)
        eb.append(first + within)
    return (np.concatenate(ea), np.concatenate(eb)) if ea else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def components(n, a, b):
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        g = coo_matrix((np.ones(a.shape[0], dtype=np.int8), (a, b)), shape=(n, n))
        return roots_from_labels(connected_components(g, directed=False)[1])
    except ImportError:
        lab = np.arange(n, dtype=np.int64)
        while True:
            new = lab.copy()
            np.minimum.at(new, a, lab[b])
            np.minimum.at(new, b, lab[a])
            while True:                                           # pointer jumping
                nxt = new[new]
                if (nxt == new).all():
                    break
                new = nxt
            if (new == lab).all():
                return lab.astype(np.int32)
            lab = new


def reduce_vectorised(root, start, end, imax, cell, wq):
    root = np.asarray(root, dtype=np.int64)
    n = root.shape[0]
    roots = np.unique(root)
    m = roots.shape[0]
    slot = np.searchsorted(roots, root)
    d = np.asarray(end, dtype=np.int64) - np.asarray(start, dtype=np.int64) + 1
    out = {}
    out["n_events"] = np.bincount(slot, minlength=m).astype(np.int32)
    C = int(cell.max()) + 1 if n else 1
    pairs = np.unique(slot * C + cell)
    out["n_cells"] = np.bincount(pairs // C, minlength=m).astype(np.int32)
    order = np.argsort(slot, kind="stable")
    first = np.concatenate([[0], np.cumsum(out["n_events"])[:-1]]).astype(np.int64)
    if n:
        out["time_start"] = np.minimum.reduceat(np.asarray(start)[order], first).astype(np.int32)
        out["time_end"] = np.maximum.reduceat(np.asarray(end)[order], first).astype(np.int32)
        out["cell_days"] = np.add.reduceat(d[order], first)
        out["area_days_q"] = np.add.reduceat((np.asarray(wq, dtype=np.int64)[cell] * d)[order], first)
        v = np.asarray(imax, dtype=np.float64) + 0.0
        nan = np.isnan(v)
        v2 = np.where(nan, 0.0, v)
        best = np.lexsort((np.arange(n), -v2, nan, slot))[first]  # per slot: non-NaN first, largest, smallest row
        out["peak_row"] = np.where(nan[best], -1, best).astype(np.int32)
        out["intensity_max"] = np.where(nan[best], np.nan, v[best])
    else:
        out.update(time_start=np.zeros(0, np.int32), time_end=np.zeros(0, np.int32), cell_days=np.zeros(0, np.int64),
                   area_days_q=np.zeros(0, np.int64), peak_row=np.zeros(0, np.int32), intensity_max=np.zeros(0))
    return out


def objects_edges(start, end, imax, offsets, nbr, gap, wq):
    n = len(start)
    a, b = edge_list(start, end, offsets, nbr, gap)
    root = components(n, a, b) if n else np.zeros(0, dtype=np.int32)
    return dict(root=root, **reduce_vectorised(root, start, end, imax, _cells(offsets), wq))


def same_result(got, want):
    """exact equality of two stage results (NaN where NaN)"""
    import numpy.testing as npt
    npt.assert_array_equal(got["root"], want["root"])
    for k in PER_OBJECT:
        assert got[k].dtype == want[k].dtype, k
        npt.assert_array_equal(got[k], want[k], err_msg=k)
