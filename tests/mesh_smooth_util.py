"""Yardstick of the mesh smoothing tests (csrc/mesh_smooth.hip): a numpy restatement written from include/dgs_mesh_smooth.h alone, and
one raw caller of the C ABI that surrounds the output, the counts and the workspace with guard bytes.

Restatement: the neighbour multiset is the list of (vertex, other corner) pairs of the valid, non-null faces; Q is np.rint (ties to
even) of a float64 product, S an int64 np.add.at, which is exact in any order; numpy float64 rounds every operation on its own and
astype(np.float32) rounds to nearest even -- so every output byte is compared exactly.
Reads nothing outside the repository."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mesh_clean_util import BAND, _guarded, _guards_intact, fans, level_set, strip  # noqa: E402,F401

ONE = 4294967296.0                                                           # 2^32
CLAMP = 32768.0
CAP = 16384                                                                  # the header's incidence cap
THREAD_MAX = 48                                                              # csrc/mesh_smooth.hip: c_v <= 48 a thread, above a wave


def incidence(V, faces):
    """The header up to `incidence` -> dict(invalid, null: numbers of faces; c [V] int64; own, other: the flat pairs (v, u in N_v))."""
    f = faces.astype(np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < V)).all(axis=1)
    null = valid & ((f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2]))
    live = f[valid & ~null]
    c = np.bincount(live.reshape(-1), minlength=V).astype(np.int64) if V else np.zeros(0, np.int64)
    own = np.concatenate((live[:, 0], live[:, 0], live[:, 1], live[:, 1], live[:, 2], live[:, 2]))
    other = np.concatenate((live[:, 1], live[:, 2], live[:, 0], live[:, 2], live[:, 0], live[:, 1]))
    return dict(invalid=int((~valid).sum()), null=int(null.sum()), c=c, own=own, other=other)


def one_pass(p, inc, moving, w):
    """pass(w) of the header on float32 [V, 3] -> float32 [V, 3]."""
    if w == 0:                                                               # the identity, not run
        return p
    q = np.rint(np.minimum(np.maximum(p.astype(np.float64), -CLAMP), CLAMP) * ONE).astype(np.int64)
    S = np.zeros(p.shape, dtype=np.int64)
    np.add.at(S, inc["own"], q[inc["other"]])
    here = p[moving].astype(np.float64)
    m = S[moving].astype(np.float64) / ((2 * inc["c"][moving]).astype(np.float64) * ONE)[:, None]
    out = p.copy()
    out[moving] = (here + np.float64(w) * (m - here)).astype(np.float32)
    return out


def restatement(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None):
    """include/dgs_mesh_smooth.h -> dict(vertices float32 [V, 3], counts [4])."""
    p = np.array(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V = p.shape[0]
    inc = incidence(V, faces)
    c = inc["c"]
    moving = (c >= 1) & (c <= CAP)
    if fixed is not None:
        moving &= np.asarray(fixed).reshape(-1) == 0
    keep = moving[inc["own"]]                                                # only the moving vertices' sums are used
    inc = dict(inc, own=inc["own"][keep], other=inc["other"][keep])
    for _ in range(iterations):
        p = one_pass(p, inc, moving, lam)
        p = one_pass(p, inc, moving, mu)
    return dict(vertices=p, counts=[inc["invalid"], inc["null"], int((c > CAP).sum()), int((c == 0).sum())])


# ---- the C ABI, raw, with guard bands ----
def make_args(L, vertices, faces, iterations, lam, mu, fixed, ws_ptr, ws_bytes, counts_ptr, out_ptr):
    from dgs_amd import _native
    a = _native.DgsMeshSmoothArgs()
    a.V, a.F = vertices.shape[0], faces.shape[0]
    a.vertices = ctypes.c_void_p(vertices.data_ptr()) if a.V else None
    a.faces = ctypes.c_void_p(faces.data_ptr()) if a.F else None
    a.fixed = ctypes.c_void_p(fixed.data_ptr()) if fixed is not None and a.V else None
    a.lam, a.mu, a.iterations = lam, mu, iterations
    a.counts, a.out_vertices = ctypes.c_void_p(counts_ptr), ctypes.c_void_p(out_ptr)
    a.workspace, a.workspace_bytes = ctypes.c_void_p(ws_ptr), ws_bytes
    return a


def smooth_raw(L, vertices, faces, device, iterations=10, lam=0.5, mu=-0.53, fixed=None):
    """dgs_mesh_smooth on numpy inputs -> dict(vertices, counts) as numpy, after asserting that the 0xA5 guards around the workspace,
    the counts and out_vertices are intact and that the inputs kept their bytes."""
    v = torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device)            # copies: the fixtures are read-only
    f = torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device)
    m = None if fixed is None else torch.from_numpy(np.array(fixed, dtype=np.uint8).reshape(-1)).to(device)
    V, F = v.shape[0], f.shape[0]
    need = L.dgs_mesh_smooth_workspace_bytes(V, F)
    assert need > 0 and need % 16 == 0
    ws, ws_ptr = _guarded(need, device)
    cnt, cnt_ptr = _guarded(16, device)
    ov, ov_ptr = _guarded(12 * V, device)
    a = make_args(L, v, f, iterations, lam, mu, m, ws_ptr, need, cnt_ptr, ov_ptr)
    assert L.dgs_mesh_smooth(ctypes.byref(a), None) == 0
    if device != "cpu":
        torch.cuda.synchronize()
    assert _guards_intact(ws, need) and _guards_intact(cnt, 16) and _guards_intact(ov, 12 * V)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), np.array(vertices, dtype=np.float32).reshape(-1, 3).view(np.uint32))
    assert np.array_equal(f.cpu().numpy(), np.array(faces, dtype=np.int32).reshape(-1, 3))
    take = lambda t, k, dt: t.cpu().numpy()[BAND:BAND + k].copy().view(dt)
    return dict(vertices=take(ov, 12 * V, np.float32).reshape(-1, 3), counts=take(cnt, 16, np.uint32).tolist())


def assert_identical(got, want):
    """Exactly: the four counts, the vertices as bit patterns."""
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])
    assert got["vertices"].shape == want["vertices"].shape
    a, b = np.ascontiguousarray(got["vertices"]).view(np.uint32), np.ascontiguousarray(want["vertices"]).view(np.uint32)
    assert np.array_equal(a, b), f"{int((a != b).any(axis=1).sum())} of {a.shape[0]} rows differ"


def voxel_ball():
    """The level set at 0.5 of the 0/1 occupancy of a ball of radius 8.2 about (11.3, 11.6, 11.2) on a 24^3 grid: voxel staircases.
    -> (vertices, faces, centre)."""
    import mesh_util as MU
    x, y, z = np.meshgrid(*(np.arange(24, dtype=np.float64),) * 3, indexing="ij")
    occ = ((x - 11.3) ** 2 + (y - 11.6) ** 2 + (z - 11.2) ** 2 < 8.2 ** 2).astype(np.float32)
    v, t = MU.restatement(occ, 0.5)
    return v, t, np.array([11.3, 11.6, 11.2])


def radius_stats(vertices, centre):
    r = np.sqrt(((vertices.astype(np.float64) - centre) ** 2).sum(axis=1))
    return float(r.mean()), float(r.std())
