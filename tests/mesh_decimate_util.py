"""Yardstick of the mesh decimation tests (csrc/mesh_decimate.hip): a numpy restatement written from include/dgs_mesh_decimate.h alone,
the bisection of consumers.decimate_mesh restated, and one raw caller of the C ABI that surrounds every output and the workspace with
guard bytes.

Restatement: numpy float64 rounds every operation on its own, np.rint rounds ties to even, the sums of the offsets are int64, and
np.unique(..., axis=0, return_index=True) gives the first, that is the smallest-index, row of each set of equal rows -- so cells,
offsets, positions and every keep / drop decision, and with them every output byte, are compared exactly.
Reads nothing outside the repository."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mesh_clean_util import BAND, _guarded, _guards_intact, blob_field, level_set, strip, tetrahedron  # noqa: E402,F401

ONE = 1048576.0                                                              # 2^20


def cells_of(vertices, faces, n):
    """The header up to `cell` -> None when nothing is output (no valid face, or ext == 0), else dict(valid [F], ref: the referenced
    vertices ascending, lo [3] float64, inv, c [len(ref), 3] int64, q likewise, cell [len(ref)])."""
    V = vertices.shape[0]
    f = faces.astype(np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < V)).all(axis=1)
    if not valid.any():
        return None, valid
    ref = np.unique(f[valid])
    pts = vertices[ref]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    assert lo.dtype == np.float32
    ext = (hi.astype(np.float64) - lo.astype(np.float64)).max()
    if ext == 0:
        return None, valid
    inv = np.float64(n) / ext
    u = (pts.astype(np.float64) - lo.astype(np.float64)) * inv
    c = np.minimum(n - 1, np.floor(u).astype(np.int64))
    q = np.rint((u - c.astype(np.float64)) * ONE).astype(np.int64)
    assert q.min() >= 0 and q.max() <= 1 << 20
    cell = (c[:, 0] * n + c[:, 1]) * n + c[:, 2]
    return dict(ref=ref, lo=lo.astype(np.float64), inv=inv, c=c, q=q, cell=cell), valid


def restatement(vertices, faces, n):
    """include/dgs_mesh_decimate.h -> dict(vertices, faces, counts [5], cells: the cell index of each output vertex, occupied: the
    number of occupied cells)."""
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = vertices.shape[0], faces.shape[0]
    g, valid = cells_of(vertices, faces, n)
    invalid = int((~valid).sum())
    if g is None:
        return dict(vertices=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), counts=[0, 0, F - invalid, 0, invalid],
                    cells=np.zeros(0, np.int64), occupied=0)
    cell_of_vertex = np.full(V, -1, dtype=np.int64)
    cell_of_vertex[g["ref"]] = g["cell"]
    fv = faces.astype(np.int64)[valid]
    fc = cell_of_vertex[fv]                                                  # [valid faces, 3] cells of the corners
    degenerate = (fc[:, 0] == fc[:, 1]) | (fc[:, 0] == fc[:, 2]) | (fc[:, 1] == fc[:, 2])
    live = np.flatnonzero(~degenerate)                                       # ascending input order among the valid faces
    _, first = np.unique(np.sort(fc[live], axis=1), axis=0, return_index=True)
    kept = live[np.sort(first)]                                              # of each set of duplicates the smallest index; input order
    kept_cells = fc[kept]                                                    # corner order unchanged
    out_cells = np.unique(kept_cells)                                        # ascending cell index
    # clusters: every referenced vertex of the cell, whether or not its faces stay
    order = np.argsort(g["cell"], kind="stable")
    sorted_cell = g["cell"][order]
    starts = np.flatnonzero(np.concatenate(([True], sorted_cell[1:] != sorted_cell[:-1])))
    occupied_cells = sorted_cell[starts]
    count = np.diff(np.concatenate((starts, [sorted_cell.shape[0]])))
    total = np.add.reduceat(g["q"][order], starts, axis=0)                   # int64 [clusters, 3]
    c_of = g["c"][order][starts]
    pick = np.searchsorted(occupied_cells, out_cells)
    assert np.array_equal(occupied_cells[pick], out_cells)
    mean = total[pick].astype(np.float64) / (count[pick].astype(np.float64) * ONE)[:, None]
    inside = c_of[pick].astype(np.float64) + mean
    p = (g["lo"][None, :] + inside / g["inv"]).astype(np.float32)
    out_faces = np.searchsorted(out_cells, kept_cells).astype(np.int32).reshape(-1, 3)
    counts = [int(out_cells.shape[0]), int(kept.shape[0]), int(degenerate.sum()), int(live.shape[0] - kept.shape[0]), invalid]
    return dict(vertices=p, faces=out_faces, counts=counts, cells=out_cells, occupied=int(occupied_cells.shape[0]))


def bisect(faces_at, F, target, n_max=1024):
    """consumers.decimate_mesh's choice of n restated; faces_at(n) -> F'(n).  -> (n, the grid sizes counted, in order); n = 0: the inputs
    come back."""
    if target <= 0 or F <= target:
        return 0, []
    lo, hi, asked = 1, n_max + 1, []
    while hi - lo > 1:
        mid = (lo + hi) // 2
        asked.append(mid)
        if faces_at(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo, asked


# ---- the C ABI, raw, with guard bands ----
def make_args(L, vertices, faces, n, ws_ptr, ws_bytes, counts_ptr):
    from dgs_amd import _native
    a = _native.DgsMeshDecimateArgs()
    a.V, a.F = vertices.shape[0], faces.shape[0]
    a.vertices = ctypes.c_void_p(vertices.data_ptr()) if a.V else None
    a.faces = ctypes.c_void_p(faces.data_ptr()) if a.F else None
    a.n = n
    a.counts, a.workspace, a.workspace_bytes = ctypes.c_void_p(counts_ptr), ctypes.c_void_p(ws_ptr), ws_bytes
    return a


def decimate_raw(L, vertices, faces, n, device, max_vertices=None, max_faces=None):
    """dgs_mesh_decimate_count + dgs_mesh_decimate_emit on numpy inputs -> dict(vertices, faces, counts) as numpy, after asserting that
    the 0xA5 guards around the workspace, the counts and both outputs are intact and that nothing past the rows the call may write
    (min(V', max_vertices), min(F', max_faces)) was touched."""
    v = torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device)            # copies: the fixtures are read-only
    f = torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device)
    V, F = v.shape[0], f.shape[0]
    need = L.dgs_mesh_decimate_workspace_bytes(V, F, n)
    assert need > 0 and need % 16 == 0
    ws, ws_ptr = _guarded(need, device)
    cnt, cnt_ptr = _guarded(20, device)
    a = make_args(L, v, f, n, ws_ptr, need, cnt_ptr)
    assert L.dgs_mesh_decimate_count(ctypes.byref(a), None) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    counts = cnt.cpu().numpy()[BAND:BAND + 20].copy().view(np.uint32).tolist()
    nv, nf = counts[0], counts[1]
    assert nv <= V and nf <= F, counts
    cap_v = nv if max_vertices is None else max_vertices
    cap_f = nf if max_faces is None else max_faces
    wrote_v, wrote_f = min(nv, cap_v), min(nf, cap_f)
    ov, ov_ptr = _guarded(12 * nv, device)                                  # room for the full result; the call may use cap rows of it
    of, of_ptr = _guarded(12 * nf, device)
    a.out_vertices, a.out_faces = ctypes.c_void_p(ov_ptr), ctypes.c_void_p(of_ptr)
    a.max_vertices, a.max_faces = cap_v, cap_f
    assert L.dgs_mesh_decimate_emit(ctypes.byref(a), None) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    assert _guards_intact(ws, need) and _guards_intact(cnt, 20)
    assert _guards_intact(ov, 12 * wrote_v) and _guards_intact(of, 12 * wrote_f)
    take = lambda t, k, dt: t.cpu().numpy()[BAND:BAND + k].copy().view(dt)
    return dict(vertices=take(ov, 12 * wrote_v, np.float32).reshape(-1, 3), faces=take(of, 12 * wrote_f, np.int32).reshape(-1, 3), counts=counts)


def count_raw(L, vertices, faces, n, device):
    """dgs_mesh_decimate_count alone -> the five counts."""
    v = torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device)
    f = torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device)
    need = L.dgs_mesh_decimate_workspace_bytes(v.shape[0], f.shape[0], n)
    ws, ws_ptr = _guarded(need, device)
    cnt, cnt_ptr = _guarded(20, device)
    a = make_args(L, v, f, n, ws_ptr, need, cnt_ptr)
    assert L.dgs_mesh_decimate_count(ctypes.byref(a), None) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    assert _guards_intact(ws, need) and _guards_intact(cnt, 20)
    return cnt.cpu().numpy()[BAND:BAND + 20].copy().view(np.uint32).tolist()


def assert_identical(got, want):
    """Exactly: the five counts, faces element by element, vertices as bit patterns."""
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"])
    assert got["vertices"].shape == want["vertices"].shape
    assert np.array_equal(np.ascontiguousarray(got["vertices"]).view(np.uint32), np.ascontiguousarray(want["vertices"]).view(np.uint32))


def assert_sound(vertices, faces, n, out):
    """The properties of an output that do not trust the restatement (`out` may be the device's result or the restatement's)."""
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    ov, of, counts = out["vertices"], out["faces"].astype(np.int64), out["counts"]
    assert counts[0] == ov.shape[0] and counts[1] == of.shape[0]
    assert counts[1] + counts[2] + counts[3] + counts[4] == faces.shape[0]                          # the counts add up
    if of.shape[0] == 0:
        assert ov.shape[0] == 0
        return
    assert of.min() >= 0 and of.max() < ov.shape[0]
    assert not ((of[:, 0] == of[:, 1]) | (of[:, 0] == of[:, 2]) | (of[:, 1] == of[:, 2])).any()    # no face with two equal indices
    assert np.unique(np.sort(of, axis=1), axis=0).shape[0] == of.shape[0]                          # no two faces share an unordered index set
    assert np.array_equal(np.unique(of), np.arange(ov.shape[0]))                                   # every output vertex is referenced
    V = vertices.shape[0]
    f = faces.astype(np.int64)
    ref = np.unique(f[((f >= 0) & (f < V)).all(axis=1)])
    lo, hi = vertices[ref].min(axis=0), vertices[ref].max(axis=0)
    assert (ov >= np.nextafter(lo, np.float32(-np.inf))).all() and (ov <= np.nextafter(hi, np.float32(np.inf))).all()   # inside the box, one ulp wider
    # The cells recomputed from the output positions ascend strictly.  A cluster's mean lies in its own closed cell, and the fp32
    # rounding of the position can carry it at most one ulp across a face of the cell: so per axis the cells of u - tol and u + tol
    # are the candidates, and some choice among them must ascend strictly (taking the smallest candidate above the last one finds
    # it if there is one).
    inv = np.float64(n) / (hi.astype(np.float64) - lo.astype(np.float64)).max()
    u = (ov.astype(np.float64) - lo.astype(np.float64)) * inv
    tol = np.float64(np.spacing(np.abs(np.concatenate((lo, hi))).max())) * inv + 2.0 ** -40
    a = np.clip(np.floor(u - tol).astype(np.int64), 0, n - 1)
    b = np.clip(np.floor(u + tol).astype(np.int64), 0, n - 1)
    cand = np.stack([((x[:, 0] * n) + y[:, 1]) * n + z[:, 2] for x in (a, b) for y in (a, b) for z in (a, b)], axis=1)
    last = -1
    for row in np.sort(cand, axis=1).tolist():
        above = [x for x in row if x > last]
        assert above, "the output vertices are not in ascending cell order"
        last = above[0]
    occupied = np.unique(_cells_plain(vertices[ref], lo, inv, n)).shape[0]
    assert ov.shape[0] <= occupied


def _cells_plain(pts, lo, inv, n):
    c = np.minimum(n - 1, np.floor((pts.astype(np.float64) - lo.astype(np.float64)) * inv).astype(np.int64))
    return (c[:, 0] * n + c[:, 1]) * n + c[:, 2]
