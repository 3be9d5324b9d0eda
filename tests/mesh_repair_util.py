"""Yardstick of the mesh repair tests (csrc/mesh_repair.hip): a numpy restatement written from include/dgs_mesh_repair.h alone, the
census restated the same way, the meshes, and raw callers of the C ABI that surround every output and the workspace with guard bytes.

Restatement: area2 in numpy float64, which rounds every operation on its own as the header demands; duplicates and edges grouped with
np.unique; the two largest keys of an edge with np.maximum.at on uint64; fans by min-label propagation with pointer jumping over the
corner ids (a fixed point has one label per class, a member that is <= every member, hence the class's smallest corner id).  The fans
are joined through the edges that have exactly two SURVIVING faces, recounted after step 3 -- the header's words, not the kernels' best
and second -- so every output byte and all counts are compared exactly.
Reads nothing outside the repository."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mesh_clean_util import BAND, _guarded, _guards_intact, level_set, strip, tetrahedron  # noqa: E402,F401

COUNTS = ("vertices", "faces", "invalid_faces", "null_faces", "duplicate_faces", "non_manifold_edges", "faces_removed",
          "non_manifold_vertices", "vertices_added", "unreferenced_vertices")
TOPOLOGY = ("border_edges", "manifold_edges", "non_manifold_edges", "non_manifold_vertices", "referenced_vertices", "faces",
            "euler_characteristic")
NONE = np.int64(0xFFFFFFFF)


def area2(v, f):
    """The header's area2 of the faces f int64 [n, 3] (valid indices) -> float64 [n]."""
    p = v.astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        u, w = b - a, c - a
        nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        return (nx * nx + ny * ny) + nz * nz


def min_labels(n, p, q):
    """The smallest member of each class of {0 .. n - 1} under the pairs (p[i], q[i]) -> int64 [n]."""
    lab = np.arange(n, dtype=np.int64)
    while p.size:
        low = np.minimum(lab[p], lab[q])
        new = lab.copy()
        for t in (p, q, lab[p], lab[q]):
            np.minimum.at(new, t, low)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def edges_of(fl, idx):
    """The 3 len(idx) edge sides of the faces idx of fl int64 [F, 3] -> dict(eid: dense edge number, n: edges, face, at_lo / at_hi: the
    face's corner ids at the edge's smaller / larger vertex, lo, hi)."""
    face = np.repeat(idx, 3)
    k = np.tile(np.arange(3), idx.shape[0])
    a, b = fl[face, k], fl[face, (k + 1) % 3]
    ca, cb = 3 * face + k, 3 * face + (k + 1) % 3
    swap = a > b
    lo, hi = np.where(swap, b, a), np.where(swap, a, b)
    at_lo, at_hi = np.where(swap, cb, ca), np.where(swap, ca, cb)
    uniq, eid = np.unique(lo * (1 << 32) + hi, return_inverse=True)
    return dict(eid=eid.reshape(-1), n=uniq.shape[0], face=face, at_lo=at_lo, at_hi=at_hi, lo=lo, hi=hi)


def fans_of(V, fl, idx):
    """Step 4 over the faces idx, joined through the edges that exactly two of them share -> dict(lab [3 F] corner labels, roots: the
    fans' labels ascending, root_vertex, vmin [V] (NONE: unreferenced), fans [V]: fans of each vertex, m: incidence of each edge)."""
    F = fl.shape[0]
    e = edges_of(fl, idx)
    m = np.bincount(e["eid"], minlength=e["n"])
    two = np.flatnonzero(m[e["eid"]] == 2)
    two = two[np.argsort(e["eid"][two], kind="stable")].reshape(-1, 2)       # the two sides of each such edge
    p = np.concatenate((e["at_lo"][two[:, 0]], e["at_hi"][two[:, 0]]))
    q = np.concatenate((e["at_lo"][two[:, 1]], e["at_hi"][two[:, 1]]))
    lab = min_labels(3 * F, p, q)
    corners = (3 * idx[:, None] + np.arange(3)[None, :]).reshape(-1)
    roots = np.unique(lab[corners])
    root_vertex = fl.reshape(-1)[roots]
    vmin = np.full(V, NONE, dtype=np.int64)
    np.minimum.at(vmin, root_vertex, roots)
    return dict(lab=lab, roots=roots, root_vertex=root_vertex, vmin=vmin, fans=np.bincount(root_vertex, minlength=V), m=m)


def census(V, faces):
    """`7 census` of the header -> dict(numbers: the seven in order, fans [V]: the fans of each vertex)."""
    fl = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((fl >= 0) & (fl < V)).all(axis=1) & (fl[:, 0] != fl[:, 1]) & (fl[:, 0] != fl[:, 2]) & (fl[:, 1] != fl[:, 2])
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return dict(numbers=[0] * 7, fans=np.zeros(V, np.int64))
    fan = fans_of(V, fl, idx)
    m = fan["m"]
    border, manifold, non = int((m == 1).sum()), int((m == 2).sum()), int((m >= 3).sum())
    ref = int((fan["fans"] > 0).sum())
    return dict(numbers=[border, manifold, non, int((fan["fans"] >= 2).sum()), ref, int(idx.size), ref - (border + manifold + non) + int(idx.size)],
                fans=fan["fans"])


def restatement(vertices, faces):
    """include/dgs_mesh_repair.h steps 1 to 6 -> dict(vertices, faces, counts [10], after_edges: the faces that survive step 3, int32
    [n, 3] with the input's indices)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = v.shape[0], f.shape[0]
    fl = f.astype(np.int64)
    valid = ((fl >= 0) & (fl < V)).all(axis=1)
    distinct = valid & (fl[:, 0] != fl[:, 1]) & (fl[:, 0] != fl[:, 2]) & (fl[:, 1] != fl[:, 2])
    a2 = np.full(F, np.nan)
    a2[distinct] = area2(v, fl[distinct])
    with np.errstate(invalid="ignore"):
        cand = distinct & (a2 > 0)
    null = valid & ~cand
    live = np.zeros(F, dtype=bool)
    idx = np.flatnonzero(cand)
    if idx.size:                                                             # 2: the smallest index of each set of three vertices
        _, inv = np.unique(np.sort(fl[idx], axis=1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        first = np.full(int(inv.max()) + 1, F, dtype=np.int64)
        np.minimum.at(first, inv, idx)
        live[first] = True
    dup = cand & ~live
    with np.errstate(over="ignore", invalid="ignore"):
        bits = a2.astype(np.float32).view(np.uint32).astype(np.uint64)
    key = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(F, dtype=np.uint64))
    marked = np.zeros(F, dtype=bool)
    non_edges = 0
    idx = np.flatnonzero(live)
    if idx.size:                                                             # 3
        e = edges_of(fl, idx)
        m = np.bincount(e["eid"], minlength=e["n"])
        k = key[e["face"]]
        best = np.zeros(e["n"], dtype=np.uint64)
        np.maximum.at(best, e["eid"], k)
        rest = k != best[e["eid"]]
        second = np.zeros(e["n"], dtype=np.uint64)
        np.maximum.at(second, e["eid"][rest], k[rest])
        out = (m[e["eid"]] >= 3) & rest & (k != second[e["eid"]])
        marked[e["face"][out]] = True
        non_edges = int((m >= 3).sum())
    survive = live & ~marked
    idx = np.flatnonzero(survive)
    counts = [0, int(idx.size), int((~valid).sum()), int(null.sum()), int(dup.sum()), non_edges, int(marked.sum()), 0, 0, V]
    if idx.size == 0:
        return dict(vertices=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), counts=counts, after_edges=f[:0])
    fan = fans_of(V, fl, idx)                                                # 4
    assert int(fan["m"].max()) <= 2                                          # one round is enough
    vmin = fan["vmin"]
    ref = vmin != NONE
    secondary = fan["roots"][vmin[fan["root_vertex"]] != fan["roots"]]       # ascending: the order of the copies
    sec_vertex = fl.reshape(-1)[secondary]
    row_of_vertex = np.cumsum(ref) - 1
    vref = int(ref.sum())
    corners = 3 * idx[:, None] + np.arange(3)[None, :]
    r, cv = fan["lab"][corners], fl[idx]
    rows = np.where(r == vmin[cv], row_of_vertex[cv], vref + np.searchsorted(secondary, r))
    counts[0], counts[7], counts[8], counts[9] = vref + int(secondary.size), int(np.unique(sec_vertex).size), int(secondary.size), V - vref
    return dict(vertices=np.concatenate((v[ref], v[sec_vertex])), faces=rows.astype(np.int32), counts=counts, after_edges=f[idx])


# ---- the C ABI, raw, with guard bands ----
def make_args(L, vertices, faces, ws_ptr, ws_bytes, counts_ptr=None, topology_ptr=None):
    from dgs_amd import _native
    a = _native.DgsMeshRepairArgs()
    a.V, a.F = vertices.shape[0], faces.shape[0]
    a.vertices = ctypes.c_void_p(vertices.data_ptr()) if a.V else None
    a.faces = ctypes.c_void_p(faces.data_ptr()) if a.F else None
    a.counts = ctypes.c_void_p(counts_ptr) if counts_ptr else None
    a.topology = ctypes.c_void_p(topology_ptr) if topology_ptr else None
    a.workspace, a.workspace_bytes = ctypes.c_void_p(ws_ptr), ws_bytes
    return a


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def repair_raw(L, vertices, faces, device):
    """dgs_mesh_repair_count + dgs_mesh_repair_emit on numpy inputs -> dict(vertices, faces, counts) as numpy, after asserting that the
    0xA5 guards around the workspace, the counts and both outputs are intact and that the inputs kept their bytes."""
    vin, fin = np.array(vertices, dtype=np.float32).reshape(-1, 3), np.array(faces, dtype=np.int32).reshape(-1, 3)
    v, f = torch.from_numpy(vin.copy()).to(device), torch.from_numpy(fin.copy()).to(device)
    V, F = v.shape[0], f.shape[0]
    need = L.dgs_mesh_repair_workspace_bytes(V, F)
    assert need > 0 and need % 16 == 0
    ws, ws_ptr = _guarded(need, device)
    cnt, cnt_ptr = _guarded(40, device)
    a = make_args(L, v, f, ws_ptr, need, cnt_ptr)
    assert L.dgs_mesh_repair_count(ctypes.byref(a), None) == 0
    _sync(device)
    counts = cnt.cpu().numpy()[BAND:BAND + 40].copy().view(np.uint32).tolist()
    nv, nf = counts[0], counts[1]
    assert nv <= V + 3 * F and nf <= F, counts
    ov, ov_ptr = _guarded(12 * nv, device)
    of, of_ptr = _guarded(12 * nf, device)
    a.out_vertices, a.out_faces, a.max_vertices, a.max_faces = ctypes.c_void_p(ov_ptr), ctypes.c_void_p(of_ptr), nv, nf
    assert L.dgs_mesh_repair_emit(ctypes.byref(a), None) == 0
    _sync(device)
    assert _guards_intact(ws, need) and _guards_intact(cnt, 40) and _guards_intact(ov, 12 * nv) and _guards_intact(of, 12 * nf)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), vin.view(np.uint32)) and np.array_equal(f.cpu().numpy(), fin)
    take = lambda t, n, dt: t.cpu().numpy()[BAND:BAND + n].copy().view(dt)
    return dict(vertices=take(ov, 12 * nv, np.float32).reshape(-1, 3), faces=take(of, 12 * nf, np.int32).reshape(-1, 3), counts=counts)


def topology_raw(L, V, faces, device):
    """dgs_mesh_topology on numpy faces (no coordinates: `vertices` is NULL) -> the seven numbers."""
    fin = np.array(faces, dtype=np.int32).reshape(-1, 3)
    f = torch.from_numpy(fin.copy()).to(device)
    need = L.dgs_mesh_repair_workspace_bytes(V, f.shape[0])
    assert need > 0 and need % 16 == 0
    ws, ws_ptr = _guarded(need, device)
    out, out_ptr = _guarded(56, device)
    a = make_args(L, torch.zeros((0, 3)), f, ws_ptr, need, topology_ptr=out_ptr)
    a.V = V
    assert L.dgs_mesh_topology(ctypes.byref(a), None) == 0
    _sync(device)
    assert _guards_intact(ws, need) and _guards_intact(out, 56) and np.array_equal(f.cpu().numpy(), fin)
    return out.cpu().numpy()[BAND:BAND + 56].copy().view(np.int64).tolist()


def assert_identical(got, want):
    """Exactly: the ten counts, the faces element by element, the vertices as bit patterns."""
    assert list(got["counts"]) == list(want["counts"]), (got["counts"], want["counts"])
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"])
    assert got["vertices"].shape == want["vertices"].shape
    a, b = np.ascontiguousarray(got["vertices"]).view(np.uint32), np.ascontiguousarray(want["vertices"]).view(np.uint32)
    assert np.array_equal(a, b), f"{int((a != b).any(axis=1).sum())} of {a.shape[0]} rows differ"


def valid_rows(V, faces):
    fl = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    return ((fl >= 0) & (fl < V)).all(axis=1)


def triangle_multiset(vertices, faces):
    """The mesh as coordinate triangles: the sorted list of the faces' 36 bytes, corners in the stored order."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).view(np.uint32).reshape(-1, 3)
    t = v[np.asarray(faces).astype(np.int64).reshape(-1, 3)].reshape(-1, 9)
    return sorted(map(bytes, t))


# ---- meshes ----
def points(n, seed):
    """n points of default_rng(seed) in the unit cube, as float32: no three on a line, no two triangles of one area."""
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)


def tetrahedra_on_an_edge():
    """Two tetrahedra on the edge {0, 1}: (0, 1, 2, 3) and (0, 1, 4, 5).  That edge has four faces."""
    f = [[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2], [0, 1, 4], [0, 4, 5], [0, 5, 1], [1, 5, 4]]
    return points(6, 21), np.array(f, dtype=np.int32)


def book(areas="distinct", order=(0, 1, 2)):
    """Three triangles on the edge {0, 1}, the spine along z; the pages reach out 1, 2, 3 (distinct areas) or 1, 1, 1 (equal)."""
    reach = (1.0, 2.0, 3.0) if areas == "distinct" else (1.0, 1.0, 1.0)
    v = [[0, 0, 0], [0, 0, 1]] + [[r * np.cos(2.1 * k), r * np.sin(2.1 * k), 0.5] for k, r in enumerate(reach)]
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32)
    if areas != "distinct":                                                  # exactly equal: the same triangle turned about the spine by 90 degrees
        v[2:] = [[1, 0, 0.5], [0, 1, 0.5], [-1, 0, 0.5]]
    return np.array(v, dtype=np.float32), f[list(order)]


def tetrahedra_on_a_vertex(n, seed=22):
    """n tetrahedra that share vertex 0 and nothing else: 3 n + 1 vertices, 4 n faces, n fans at vertex 0."""
    v = points(3 * n + 1, seed)
    f = []
    for t in range(n):
        a, b, c = 3 * t + 1, 3 * t + 2, 3 * t + 3
        f += [[0, a, b], [0, b, c], [0, c, a], [a, c, b]]
    return v, np.array(f, dtype=np.int32)


def pinch_after_edges():
    """A closed umbrella of six faces about vertex 0 (ring 1 .. 6) whose rim edges {1, 2} and {4, 5} carry two larger triangles each
    (apexes 7, 8 and 9, 10): step 3 removes the umbrella's faces (0, 1, 2) and (0, 4, 5), the smallest on those edges, and the
    umbrella falls into two fans at vertex 0.  -> (vertices, faces, the vertex)."""
    ang = np.arange(6) * (np.pi / 3)
    ring = np.stack((np.cos(ang), np.sin(ang), np.zeros(6)), axis=1)
    far = np.array([[3.0, 2.0, 2.0], [3.0, 2.0, -2.5], [-3.0, -2.0, 2.2], [-3.0, -2.0, -2.7]])
    v = np.concatenate((np.array([[0.0, 0.0, 0.3]]), ring, far)).astype(np.float32)
    f = [[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)] + [[1, 2, 7], [2, 1, 8], [4, 5, 9], [5, 4, 10]]
    return v, np.array(f, dtype=np.int32), 0


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)
    return v, f


def one_tetrahedron():
    return points(4, 23), np.array(tetrahedron(0), dtype=np.int32)


def grid(nx, ny):
    """An open bumpy sheet of 2 nx ny faces: a border all around."""
    x, y = np.meshgrid(np.arange(nx + 1) * 1.0, np.arange(ny + 1) * 1.0, indexing="ij")
    v = np.stack((x.ravel(), y.ravel(), np.sin(x.ravel() * 1.7) * np.cos(y.ravel() * 2.3)), axis=1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).ravel()
    b, c, d = a + (ny + 1), a + (ny + 2), a + 1
    return v, np.concatenate((np.stack((a, b, c), axis=1), np.stack((a, c, d), axis=1))).astype(np.int32)


def cone(n):
    """A closed fan of n faces about vertex 0 over a ring of n vertices: one fan, n spokes of two faces, n border edges."""
    ang = np.arange(n) * (2 * np.pi / n)
    v = np.concatenate((np.array([[0.0, 0.0, 1.0]]), np.stack((np.cos(ang), np.sin(ang), np.zeros(n)), axis=1))).astype(np.float32)
    i = np.arange(n)
    return v, np.stack((np.zeros(n, dtype=np.int64), 1 + i, 1 + (i + 1) % n), axis=1).astype(np.int32)


def voxel_ball():
    from mesh_smooth_util import voxel_ball as ball
    v, f, _ = ball()
    return v, f


def slab(nx=24, ny=6, thickness=0.3, tilt=0.25):
    """A thin closed slab: two parallel sheets of nx x ny squares, `thickness` apart, joined at the rim; it rises by `tilt` a unit of
    x, so that the cells of a clustering grid cut through it at a shallow angle.  The unit is the square's side.  Closed and manifold."""
    x, y = np.meshgrid(np.arange(nx + 1) * 1.0, np.arange(ny + 1) * 1.0, indexing="ij")
    x, y = x.ravel(), y.ravel()
    low = np.stack((x, y, tilt * x), axis=1)
    v = np.concatenate((low, low + np.array([0.0, 0.0, thickness]))).astype(np.float32)
    n = (nx + 1) * (ny + 1)
    at = lambda i, j: i * (ny + 1) + j
    f = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            f += [[a, c, b], [a, d, c], [n + a, n + b, n + c], [n + a, n + c, n + d]]
    rim = [at(i, 0) for i in range(nx)] + [at(nx, j) for j in range(ny)] + [at(i, ny) for i in range(nx, 0, -1)] + [at(0, j) for j in range(ny, 0, -1)]
    for s in range(len(rim)):
        a, b = rim[s], rim[(s + 1) % len(rim)]
        f += [[a, b, n + b], [a, n + b, n + a]]
    return v, np.array(f, dtype=np.int32)
