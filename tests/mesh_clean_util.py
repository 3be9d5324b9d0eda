"""Yardstick of the mesh clean-up tests (csrc/mesh_clean.hip): a numpy restatement written from include/dgs_mesh_clean.h alone, the
meshes, and one raw caller of the C ABI that surrounds every output and the workspace with guard bytes.

Restatement: labels by min-label propagation with pointer jumping (every round gives each vertex, and the vertex its label names, the
smallest label on any of its faces, then replaces labels by the labels' labels until that changes nothing); a fixed point has one label
per component, an index of the component that is <= each of its members, hence its smallest index.  Boxes are exact fp32 minima and
maxima; d2 = (dx * dx + dy * dy) + dz * dz in numpy float64, which rounds every operation on its own as the header demands, so the
keep / remove decisions, and with them every output byte, are compared exactly.
Reads nothing outside the repository."""
import ctypes
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_util as MU  # noqa: E402

GUARD = 0xA5
BAND = 256                                                                   # guard bytes on each side


def valid_faces(V, faces):
    f = faces.astype(np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def vertex_labels(V, faces):
    """-> (label of every vertex [V] int64, rounds): the smallest index of the vertex's component; itself where no valid face uses it."""
    fv = faces.astype(np.int64).reshape(-1, 3)[valid_faces(V, faces)]
    lab = np.arange(V, dtype=np.int64)
    flat = fv.reshape(-1)
    rounds = 0
    while fv.shape[0]:
        rounds += 1
        low = np.repeat(lab[fv].min(axis=1), 3)
        new = lab.copy()
        np.minimum.at(new, flat, low)
        np.minimum.at(new, lab[flat], low)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    return lab, rounds


def diag2(lo, hi):
    d = hi.astype(np.float64) - lo.astype(np.float64)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def components(vertices, faces):
    """-> dict(valid [F], labels [F] int32 (-1 invalid), roots [C], n [C], d2 [C], D2): the header's per-component quantities."""
    V = int(vertices.shape[0])
    valid = valid_faces(V, faces)
    lab, rounds = vertex_labels(V, faces)
    fv = faces.astype(np.int64).reshape(-1, 3)[valid]
    labels = np.full(faces.shape[0], -1, dtype=np.int32)
    labels[valid] = lab[fv[:, 0]]
    if fv.shape[0] == 0:
        e = np.zeros(0)
        return dict(valid=valid, labels=labels, roots=np.zeros(0, np.int64), n=np.zeros(0, np.int64), d2=e, D2=np.float64("nan"), rounds=rounds)
    roots, n = np.unique(labels[valid].astype(np.int64), return_counts=True)
    ref = np.unique(fv)                                                      # referenced vertices, ascending
    order = np.argsort(lab[ref], kind="stable")
    sorted_lab = lab[ref][order]
    starts = np.flatnonzero(np.concatenate(([True], sorted_lab[1:] != sorted_lab[:-1])))
    assert np.array_equal(sorted_lab[starts], roots)
    pts = vertices[ref][order]
    lo, hi = np.minimum.reduceat(pts, starts, axis=0), np.maximum.reduceat(pts, starts, axis=0)
    assert lo.dtype == np.float32
    return dict(valid=valid, labels=labels, roots=roots, n=n, d2=diag2(lo, hi), D2=diag2(vertices[ref].min(axis=0), vertices[ref].max(axis=0)),
                rounds=rounds)


def removed_by(comp, min_f, min_d):
    """-> (by face number [C], by diameter [C]) bool, each rule on its own."""
    few = comp["n"] < min_f if min_f > 0 else np.zeros(comp["n"].shape, dtype=bool)
    p = np.float64(min_d) / 100.0
    small = comp["d2"] < (p * p) * comp["D2"] if min_d > 0 else np.zeros(comp["n"].shape, dtype=bool)
    return few, small


def restatement(vertices, faces, min_f, min_d, comp=None):
    """include/dgs_mesh_clean.h -> dict(vertices, faces, labels, counts [5])."""
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V = vertices.shape[0]
    comp = comp or components(vertices, faces)
    few, small = removed_by(comp, min_f, min_d)
    kept_roots = comp["roots"][~(few | small)]
    face_kept = comp["valid"] & np.isin(comp["labels"], kept_roots)
    kept_faces = faces[face_kept].astype(np.int64)
    vertex_kept = np.zeros(V, dtype=bool)
    vertex_kept[kept_faces.reshape(-1)] = True
    new_index = np.cumsum(vertex_kept) - 1
    counts = [int(vertex_kept.sum()), int(face_kept.sum()), int(comp["roots"].shape[0]), int(kept_roots.shape[0]), int((~comp["valid"]).sum())]
    return dict(vertices=vertices[vertex_kept], faces=new_index[kept_faces].astype(np.int32).reshape(-1, 3), labels=comp["labels"], counts=counts)


# ---- the C ABI, raw, with guard bands ----
def _guarded(nbytes, device):
    """-> (whole uint8 tensor filled with GUARD, data pointer of its middle part): 16-byte aligned like the tensor itself."""
    t = torch.full((BAND + nbytes + BAND,), GUARD, dtype=torch.uint8, device=device)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + BAND


def _guards_intact(t, written):
    b = t.cpu().numpy()
    return bool((b[:BAND] == GUARD).all()) and bool((b[BAND + written:] == GUARD).all())


def make_args(L, vertices, faces, min_f, min_d, ws_ptr, ws_bytes, counts_ptr):
    from dgs_amd import _native
    a = _native.DgsMeshCleanArgs()
    a.V, a.F = vertices.shape[0], faces.shape[0]
    a.vertices = ctypes.c_void_p(vertices.data_ptr()) if a.V else None
    a.faces = ctypes.c_void_p(faces.data_ptr()) if a.F else None
    a.min_faces, a.min_diag_pct = min_f, min_d
    a.counts, a.workspace, a.workspace_bytes = ctypes.c_void_p(counts_ptr), ctypes.c_void_p(ws_ptr), ws_bytes
    return a


def clean_raw(L, vertices, faces, min_f, min_d, device, max_vertices=None, max_faces=None, labels=True):
    """dgs_mesh_clean_count + dgs_mesh_clean_emit on numpy inputs -> dict(vertices, faces, labels, counts) as numpy, after asserting that
    the 0xA5 guards around the workspace, the counts and the three outputs are intact and that nothing past the rows the call may write
    (min(V', max_vertices), min(F', max_faces)) was touched."""
    v = torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device)            # copies: the fixtures are read-only
    f = torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device)
    V, F = v.shape[0], f.shape[0]
    need = L.dgs_mesh_clean_workspace_bytes(V, F)
    assert need > 0 and need % 16 == 0
    ws, ws_ptr = _guarded(need, device)
    cnt, cnt_ptr = _guarded(20, device)
    a = make_args(L, v, f, min_f, min_d, ws_ptr, need, cnt_ptr)
    assert L.dgs_mesh_clean_count(ctypes.byref(a), None) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    counts = cnt.cpu().numpy()[BAND:BAND + 20].copy().view(np.uint32).tolist()
    nv, nf = counts[0], counts[1]
    cap_v = nv if max_vertices is None else max_vertices
    cap_f = nf if max_faces is None else max_faces
    wrote_v, wrote_f = min(nv, cap_v), min(nf, cap_f)
    ov, ov_ptr = _guarded(12 * nv, device)                                  # room for the full result; the call may use cap rows of it
    of, of_ptr = _guarded(12 * nf, device)
    ol, ol_ptr = _guarded(4 * F, device)
    a.out_vertices, a.out_faces = ctypes.c_void_p(ov_ptr), ctypes.c_void_p(of_ptr)
    a.labels = ctypes.c_void_p(ol_ptr) if labels else None
    a.max_vertices, a.max_faces = cap_v, cap_f
    assert L.dgs_mesh_clean_emit(ctypes.byref(a), None) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    assert _guards_intact(ws, need) and _guards_intact(cnt, 20)
    assert _guards_intact(ov, 12 * wrote_v) and _guards_intact(of, 12 * wrote_f) and _guards_intact(ol, 4 * F if labels else 0)
    take = lambda t, n, dt: t.cpu().numpy()[BAND:BAND + n].copy().view(dt)
    return dict(vertices=take(ov, 12 * wrote_v, np.float32).reshape(-1, 3), faces=take(of, 12 * wrote_f, np.int32).reshape(-1, 3),
                labels=take(ol, 4 * F, np.int32) if labels else None, counts=counts)


def assert_identical(got, want):
    """Exactly: the five counts, faces and labels element by element, vertices as bit patterns."""
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"])
    assert got["vertices"].shape == want["vertices"].shape
    assert np.array_equal(np.ascontiguousarray(got["vertices"]).view(np.uint32), np.ascontiguousarray(want["vertices"]).view(np.uint32))
    if got.get("labels") is not None:
        assert np.array_equal(got["labels"], want["labels"])


# ---- meshes ----
@functools.lru_cache(maxsize=None)
def level_set(name):
    """Marching-cubes fixtures of tests/mesh_util.py through its restatement -> (vertices, faces), computed once, never modified."""
    occ, level = {
        "noise24_08": lambda: (MU.noise_pair()[0], 0.8),
        "noise24_05": lambda: (MU.noise_pair()[0], 0.5),
        "noise20_closed_05": lambda: (MU.noise_pair()[1], 0.5),
        "9x33x17": lambda: (MU.shaped_noise((9, 33, 17), 3), 0.5),
        "sphere": lambda: (MU.sphere(), 0.0),
        "torus": lambda: (MU.torus(), 0.0),
        "blobs": lambda: (blob_field(), 0.5),
        "noise64_05": lambda: (MU.shaped_noise((64, 64, 64), 5), 0.5),
        "noise64_08": lambda: (MU.shaped_noise((64, 64, 64), 5), 0.8),
    }[name]()
    v, t = MU.restatement(occ, level)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def level_set_components(name):
    return components(*level_set(name))


BLOB_GRID = 40
BLOB_MIN_F, BLOB_MIN_D = 300, 25.0                                         # the thresholds test_blob_field uses


def blob_field():
    """A sum of Gaussian blobs on a 40^3 grid, level 0.5: one large ball, a compact ball (many faces, short diagonal), a thin rod (few
    faces, long diagonal) and default_rng(11) specks (few faces, short diagonal)."""
    n = BLOB_GRID
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")

    def blob(c, s):
        return np.exp(-0.5 * (((x - c[0]) / s[0]) ** 2 + ((y - c[1]) / s[1]) ** 2 + ((z - c[2]) / s[2]) ** 2))

    occ = blob((14.3, 14.6, 14.2), (7.0, 7.0, 7.0))                         # radius 7 * sqrt(2 ln 2) = 8.2
    occ += blob((32.4, 31.7, 8.3), (2.6, 2.6, 2.6))                          # radius 3.1: a compact ball
    occ += blob((20.2, 34.3, 33.6), (7.5, 0.75, 0.75))                       # half-length 8.8, radius 0.9: a rod along x
    rng = np.random.default_rng(11)
    for c in rng.uniform(26.0, 37.0, size=(6, 3)):
        c[1] -= 14.0                                                         # y in [12, 23], x, z in [26, 37]: clear of the three others
        occ += blob(c, (0.7, 0.7, 0.7))
    return occ.astype(np.float32)


def tetrahedron(base):
    return [[base, base + 1, base + 2], [base, base + 2, base + 3], [base, base + 3, base + 1], [base + 1, base + 3, base + 2]]


def strip(n_faces, order=None):
    """A triangle strip of n_faces faces on n_faces + 2 vertices along x; `order` renames vertex i to order[i] (positions move with it)."""
    n = n_faces + 2
    pos = np.stack((np.arange(n) * 0.5, (np.arange(n) % 2).astype(np.float64), np.zeros(n)), axis=1).astype(np.float32)
    i = np.arange(n_faces)
    faces = np.stack((i, i + 1, i + 2), axis=1)
    faces[1::2] = faces[1::2][:, [1, 0, 2]]
    if order is None:
        return pos, faces.astype(np.int32)
    order = np.asarray(order)
    moved = np.empty_like(pos)
    moved[order] = pos
    return moved, order[faces].astype(np.int32)


def fans(sizes, gap=3.0):
    """One triangle fan per entry of `sizes` (that many faces, size + 2 vertices), side by side along x, the k-th scaled by k + 1."""
    vs, fs, base = [], [], 0
    for k, s in enumerate(sizes):
        ang = np.linspace(0.0, np.pi, s + 1)
        ring = np.stack((np.cos(ang), np.sin(ang), np.zeros(s + 1)), axis=1) * (k + 1)
        v = np.concatenate((np.zeros((1, 3)), ring)) + np.array([gap * k * (k + 1), 0.0, 0.0])
        i = np.arange(s)
        fs.append(np.stack((np.zeros(s, dtype=np.int64), i + 1, i + 2), axis=1) + base)
        vs.append(v)
        base += s + 2
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)
