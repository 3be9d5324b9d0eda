"""Mesh decimation by vertex clustering (csrc/mesh_decimate.hip, include/dgs_mesh_decimate.h, dgs_amd.consumers.cluster_vertices /
decimate_mesh, extract_mesh(decimate_target)) on the CPU-emulated build of the kernels: every output byte and all five counts against
the numpy restatement of tests/mesh_decimate_util.py.  The checks are functions of (library, device), which
tests/test_mesh_decimate_gpu.py runs on the device.

Sizes.  Every kernel of csrc/mesh_decimate.hip runs workgroups of 256 threads, one row a thread; a wave is 64 rows, a scan block 256
rows, and the scan over the block totals gives each of its 1,024 threads one block up to 1,024 blocks.  So the strips have 63, 64, 65
faces (a wave), 255, 256, 257 (a workgroup and a scan block) and 65,537 (257 scan blocks of faces, of vertices and of clusters);
noise64_05 on the device has 3,130 blocks of faces, more than the 1,024 threads of that scan."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import field_util as FU  # noqa: E402
import mesh_decimate_util as D  # noqa: E402
from dgs_amd import _native, consumers  # noqa: E402
from dgs_amd.consumers import cluster_vertices, decimate_mesh  # noqa: E402  (without the feature the module fails here)

assert _native.MESH_DECIMATE_SYMBOLS

# (fixture, n) -> (V', F', degenerate, duplicates): figures of a CPU probe of the fixtures with the restatement
FIXTURE_STATS = {
    ("sphere", 8): (244, 484, 2032, 0),
    ("torus", 3): (9, 10, 2424, 6),
    ("blobs", 16): (329, 632, 2586, 2),
    ("noise24_05", 11): (1331, 5896, 32309, 956),
    ("noise64_05", 32): (32765, 156089, 625494, 19616),
}
# several n each; 28 and 29 on blobs, 63 and 64 on noise64_05 are steps where F'(n) falls as n grows.  noise64_05: on the device only
FIXTURE_RUNS = [("sphere", 1), ("sphere", 2), ("sphere", 8), ("sphere", 50), ("torus", 3), ("torus", 17), ("blobs", 16), ("blobs", 28),
                ("blobs", 29), ("blobs", 200), ("noise24_05", 11), ("noise24_05", 13), ("noise24_05", 64)]
NOT_MONOTONE = {"blobs": ((28, 1657), (29, 1639))}


def lib_of(device):
    if device == "cpu":
        from emu_util import emu_lib
        return emu_lib()
    return _native.lib()


def as_tensors(vertices, faces, device):
    return (torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device),
            torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device))


def check(device, vertices, faces, n):
    """The raw call against the restatement, exactly; a second call gives the same bytes; the Python call gives the same tensors; the
    properties that do not trust the restatement hold for the device's output.  -> the restatement's result."""
    L = lib_of(device)
    want = D.restatement(vertices, faces, n)
    got = D.decimate_raw(L, vertices, faces, n, device)
    print("n", n, "V", np.shape(vertices)[0], "F", np.shape(faces)[0], "counts", got["counts"], "restated", want["counts"])
    D.assert_identical(got, want)
    D.assert_identical(D.decimate_raw(L, vertices, faces, n, device), got)
    D.assert_sound(vertices, faces, n, got)
    tv, tf = as_tensors(vertices, faces, device)
    v, f, counts = cluster_vertices(tv, tf, n, return_counts=True, lib=None if device != "cpu" else L)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.device == tv.device and f.device == tv.device and not v.requires_grad
    D.assert_identical(dict(vertices=v.cpu().numpy(), faces=f.cpu().numpy(), counts=counts), want)
    return want


def test_fixture_statistics():
    """The restatement's figures of the marching-cubes fixtures, so that a drift of either shows (noise64_05: tests/test_mesh_decimate_gpu.py)."""
    for (name, n), stats in FIXTURE_STATS.items():
        if name == "noise64_05":
            continue
        v, f = D.level_set(name)
        want = D.restatement(v, f, n)
        assert tuple(want["counts"][:4]) == stats and want["counts"][4] == 0, (name, n, want["counts"])
        D.assert_sound(v, f, n, want)
    for name, steps in NOT_MONOTONE.items():                                  # F'(n) is not monotone: the bisection's docstring says so
        v, f = D.level_set(name)
        for n, faces_left in steps:
            assert D.restatement(v, f, n)["counts"][1] == faces_left
        assert steps[0][0] < steps[1][0] and steps[0][1] > steps[1][1]


def check_fixture(device, name, n):
    v, f = D.level_set(name)
    want = check(device, v, f, n)
    if (name, n) in FIXTURE_STATS:
        assert tuple(want["counts"][:4]) == FIXTURE_STATS[(name, n)]
    if n == 1:
        assert want["counts"] == [0, 0, f.shape[0], 0, 0]                    # one cell: every face is degenerate
    return want


@pytest.mark.parametrize("name,n", FIXTURE_RUNS)
def test_fixture_emulated(name, n):
    check_fixture("cpu", name, n)


# ---- hand-built cases: name -> (vertices, faces, n) ----
TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32))
FAR = 1.0e6


def _tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    return v, np.array(D.tetrahedron(0), dtype=np.int32)


def _grid(nx, ny, z=0.0, flip=False, step=1.0):
    """A sheet of nx x ny squares, two triangles each, at height z; flip reverses every triangle."""
    x, y = np.meshgrid(np.arange(nx + 1) * step, np.arange(ny + 1) * step, indexing="ij")
    v = np.stack((x.ravel(), y.ravel(), np.full(x.size, z)), axis=1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).ravel()
    b, c, d = a + (ny + 1), a + (ny + 2), a + 1
    f = np.concatenate((np.stack((a, b, c), axis=1), np.stack((a, c, d), axis=1)))
    if flip:
        f = f[:, [0, 2, 1]]
    return v, f.astype(np.int32)


def _two_sheets():
    """Two parallel sheets a hundredth of a cell apart, the second with the opposite orientation: their faces pair up as duplicates."""
    v0, f0 = _grid(6, 6, 0.25)
    v1, f1 = _grid(6, 6, 0.26, flip=True)
    return np.concatenate((v0, v1)), np.concatenate((f0, f1 + v0.shape[0])).astype(np.int32)


def _invalid_mixed():
    """A tetrahedron and a sheet, invalid faces in between, and vertices no valid face names far outside: they must not move the box."""
    tv, tf = _tetrahedron()
    gv, gf = _grid(4, 4, 2.0)
    pad = np.array([[FAR, -FAR, FAR]], dtype=np.float32)
    v = np.concatenate((pad, tv, pad * -1, gv, pad))                          # unreferenced: in front, inside, behind
    tf, gf = tf + 1, gf + 1 + tv.shape[0] + 1
    V = v.shape[0]
    bad = np.array([[-1, 1, 2], [2, V, 3], [4, 5, 2 ** 31 - 1], [-2 ** 31, -1, V], [V, V, V], [0, V, 0]], dtype=np.int32)   # the last names a far vertex but is invalid
    return v, np.concatenate((tf[:2], bad[:2], tf[2:], gf[:10], bad[2:5], gf[10:], bad[5:])).astype(np.int32)


def _at_hi():
    """x runs from 0 to 3 (the longest axis) with a vertex exactly at hi: it clamps into cell n - 1 with offset 2^20."""
    v = np.array([[0, 0, 0], [3, 0, 0], [3, 1, 0], [0, 1, 0], [1.5, 0.5, 0.75]], dtype=np.float32)
    return v, np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], dtype=np.int32)


def _ribbon(n_faces, n, order=None):
    """mesh_clean_util.strip laid out in rows of 512 vertices, half a unit apart along x and the rows two units apart, so that a long
    strip fits a grid of at most 1,024 cells with every vertex in a cell of its own; up to 510 faces it is the plain strip.  The
    faces from one row to the next are long, which no rule forbids."""
    v, f = D.strip(n_faces)
    i = np.arange(v.shape[0])
    v = np.stack((0.5 * (i % 512), (i % 2) + 2.0 * (i // 512), np.zeros(i.shape[0])), axis=1).astype(np.float32)
    if order is not None:
        moved = np.empty_like(v)
        moved[order] = v
        v, f = moved, np.asarray(order)[f].astype(np.int32)
    return v, f, n


HAND = {
    "one_triangle_n1": lambda: TRIANGLE + (1,),
    "one_triangle_n2": lambda: TRIANGLE + (2,),
    "tetrahedron_n2": lambda: _tetrahedron() + (2,),
    "tetrahedron_n7": lambda: _tetrahedron() + (7,),
    "every_face_invalid": lambda: (TRIANGLE[0], np.array([[0, 1, 3], [-1, 0, 1], [3, 3, 3]], dtype=np.int32), 4),
    "invalid_mixed_n3": lambda: _invalid_mixed() + (3,),
    "invalid_mixed_n40": lambda: _invalid_mixed() + (40,),
    "one_point": lambda: (np.full((5, 3), 0.375, dtype=np.float32), np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32), 8),
    "flat_n5": lambda: _grid(9, 4) + (5,),
    "flat_n64": lambda: _grid(9, 4) + (64,),
    "at_hi_n3": lambda: _at_hi() + (3,),
    "at_hi_n1024": lambda: _at_hi() + (1024,),
    "two_sheets": lambda: _two_sheets() + (6,),
    "strip63": lambda: _ribbon(63, 40),
    "strip64": lambda: _ribbon(64, 40),
    "strip65": lambda: _ribbon(65, 40),
    "strip255": lambda: _ribbon(255, 200),
    "strip256": lambda: _ribbon(256, 200),
    "strip257": lambda: _ribbon(257, 200),
    "strip65537": lambda: _ribbon(65537, 640),
    "strip5000_shuffled": lambda: _ribbon(5000, 640, np.random.default_rng(7).permutation(5002)),
    "blobs_n1024": lambda: D.level_set("blobs") + (1024,),
}


def check_hand(device, name):
    v, f, n = HAND[name]()
    want = check(device, v, f, n)
    V, F = v.shape[0], f.shape[0]
    nv, nf, degenerate, duplicates, invalid = want["counts"]
    if name == "one_triangle_n1":
        assert want["counts"] == [0, 0, 1, 0, 0]
    if name == "one_triangle_n2":                                             # (0,0) (1,0) (0,1) in three cells: positions are the inputs
        assert want["counts"] == [3, 1, 0, 0, 0] and np.array_equal(want["faces"], [[0, 2, 1]])
        assert np.array_equal(want["vertices"], v[[0, 2, 1]])                 # ascending cell index: (0,0,0), (0,1,0), (1,0,0)
    if name.startswith("tetrahedron"):
        assert want["counts"] == [4, 4, 0, 0, 0]
    if name == "every_face_invalid":
        assert want["counts"] == [0, 0, 0, 0, 3]
    if name.startswith("invalid_mixed"):                                      # as without the invalid faces and the far vertices
        tv, tf = _tetrahedron()
        gv, gf = _grid(4, 4, 2.0)
        alone = D.restatement(np.concatenate((tv, gv)), np.concatenate((tf, gf + 4)), n)
        assert invalid == 6 and want["counts"][:4] == alone["counts"][:4]
        assert np.array_equal(want["vertices"].view(np.uint32), alone["vertices"].view(np.uint32)) and np.array_equal(want["faces"], alone["faces"])
        assert float(np.abs(want["vertices"]).max()) <= 4.0
    if name == "one_point":                                                   # ext == 0: every valid face counts as degenerate
        assert want["counts"] == [0, 0, 2, 0, 0]
    if name == "flat_n64":                                                    # nine cells along x would do; every vertex keeps a cell of its own
        assert want["counts"] == [V, F, 0, 0, 0] and np.array_equal(want["vertices"][:, 2], np.zeros(V, np.float32))
    if name.startswith("at_hi"):
        g, _ = D.cells_of(v, f, n)
        assert int(g["c"][1, 0]) == n - 1 and int(g["q"][1, 0]) == 1 << 20 and int(g["q"][2, 0]) == 1 << 20 and int(g["q"].max()) == 1 << 20
        assert int((g["q"] == 1 << 20).sum()) == 2                            # only hi of the longest axis
        assert want["counts"] == [5, 4, 0, 0, 0] and float(want["vertices"][:, 0].max()) == 3.0
    if name == "two_sheets":                                                  # each face of the second sheet repeats one of the first: the first stays, as it was wound
        v0, f0 = _grid(6, 6, 0.25)
        first = D.restatement(v0, f0, n)
        assert nf == first["counts"][1] and degenerate == 2 * first["counts"][2] and duplicates == nf + 2 * first["counts"][3] and nf > 20
        assert np.array_equal(want["faces"], first["faces"])
        normal = np.cross(want["vertices"][want["faces"][:, 1]] - want["vertices"][want["faces"][:, 0]],
                          want["vertices"][want["faces"][:, 2]] - want["vertices"][want["faces"][:, 0]])[:, 2]
        assert bool((normal > 0).all())                                       # the orientation of the first sheet
    if name.startswith("strip") and name != "strip5000_shuffled":
        assert F == int(name[5:]) and nf > F // 2 and duplicates == 0
    if name == "blobs_n1024":                                                 # nearly an identity: marching cubes leaves a few vertices closer than a cell
        assert nv >= 0.98 * V and nf >= 0.98 * F and duplicates == 0 and nv < V
    if name in ("strip65537", "strip5000_shuffled"):                        # nearly an identity: every vertex a cluster of its own
        assert want["counts"] == [V, F, 0, 0, 0]
        assert float(np.abs(np.sort(want["vertices"].astype(np.float64), axis=0) - np.sort(v.astype(np.float64), axis=0)).max()) <= 2.0 ** -20 * float(np.abs(v).max())


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_emulated(name):
    check_hand("cpu", name)


def check_empty(device):
    L = lib_of(device)
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    some_v, some_f = _tetrahedron()
    for v, f, invalid in ((none_v, none_f, 0), (some_v, none_f, 0), (none_v, some_f, 4)):
        got = D.decimate_raw(L, v, f, 4, device)
        assert got["counts"] == [0, 0, 0, 0, invalid] and got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
        D.assert_identical(got, D.restatement(v, f, 4))
        out = cluster_vertices(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), 4, lib=None if device != "cpu" else L)
        assert tuple(out[0].shape) == (0, 3) and tuple(out[1].shape) == (0, 3) and out[0].dtype == torch.float32 and out[1].dtype == torch.int32


def test_empty_meshes_emulated():
    check_empty("cpu")


def check_limits(device):
    """max_vertices / max_faces below V' / F': the rows before them are the full result's; decimate_raw asserts that the guard bytes
    behind them, and around the workspace and the counts, keep their fill."""
    L = lib_of(device)
    v, f = D.level_set("noise24_05")
    want = D.restatement(v, f, 11)
    nv, nf = want["counts"][:2]
    assert nv > 100 and nf > 77
    for mv, mf in ((nv, nf), (100, 77), (0, 5), (3, 0), (nv + 10, nf + 10)):
        got = D.decimate_raw(L, v, f, 11, device, max_vertices=mv, max_faces=mf)
        assert got["counts"] == want["counts"]
        assert np.array_equal(got["vertices"].view(np.uint32), want["vertices"][:mv].view(np.uint32)) and np.array_equal(got["faces"], want["faces"][:mf])


def test_limits_leave_the_rest_untouched_emulated():
    check_limits("cpu")


def check_invariance(device, name, n):
    """Renaming the vertices or reordering the faces changes no output vertex byte and no count; the faces stay the same set."""
    L = lib_of(device)
    v, f = D.level_set(name)
    base = D.decimate_raw(L, v, f, n, device)
    rng = np.random.default_rng(5)
    perm = rng.permutation(v.shape[0])                                        # vertex i becomes perm[i]
    moved = np.empty_like(v)
    moved[perm] = v
    got = D.decimate_raw(L, moved, perm[f].astype(np.int32), n, device)
    D.assert_identical(got, base)                                             # the faces too: their order and their cells are unchanged
    order = rng.permutation(f.shape[0])
    got = D.decimate_raw(L, v, f[order], n, device)
    assert got["counts"] == base["counts"] and np.array_equal(got["vertices"].view(np.uint32), base["vertices"].view(np.uint32))
    as_set = lambda t: np.unique(np.sort(t, axis=1), axis=0)
    assert np.array_equal(as_set(got["faces"]), as_set(base["faces"]))
    D.assert_identical(got, D.restatement(v, f[order], n))


@pytest.mark.parametrize("name,n", [("blobs", 16), ("noise24_05", 11)])
def test_invariance_emulated(name, n):
    check_invariance("cpu", name, n)


def check_decimate_mesh(device):
    L = lib_of(device)
    lib = None if device != "cpu" else L
    for name, target, n_want in (("blobs", 1650, 29), ("noise24_05", 10000, 13), ("blobs", 1, 2)):
        v, f = D.level_set(name)
        n_restated, asked = D.bisect(lambda n: D.restatement(v, f, n)["counts"][1], f.shape[0], target)
        assert n_restated == n_want and len(asked) == 10
        assert [D.count_raw(L, v, f, n, device)[1] for n in asked[-3:]] == [D.restatement(v, f, n)["counts"][1] for n in asked[-3:]]
        tv, tf = as_tensors(v, f, device)
        ov, of, n = decimate_mesh(tv, tf, target, return_n=True, lib=lib)
        want = D.restatement(v, f, n_restated)
        print(name, "target", target, "n", n, "counts", want["counts"])
        assert n == n_restated and of.shape[0] <= target
        D.assert_identical(dict(vertices=ov.cpu().numpy(), faces=of.cpu().numpy(), counts=want["counts"]), want)
        assert ov.device == tv.device and of.dtype == torch.int32 and ov.dtype == torch.float32
        if target == 1:                                                       # an empty mesh, not an error
            assert tuple(ov.shape) == (0, 3) and tuple(of.shape) == (0, 3)
    v, f = D.level_set("blobs")
    tv, tf = as_tensors(v, f, device)
    for target in (f.shape[0], f.shape[0] + 1, 1e9, 0, -5):                   # F <= target, or no target: the inputs themselves
        out = decimate_mesh(tv, tf, target, lib=lib)
        assert out[0] is tv and out[1] is tf
    assert decimate_mesh(tv, tf, 0, return_n=True, lib=lib)[2] == 0
    ov, of, n = decimate_mesh(tv, tf, 1650, n_max=20, return_n=True, lib=lib)  # a smaller n_max bounds the search
    assert n == D.bisect(lambda k: D.restatement(v, f, k)["counts"][1], f.shape[0], 1650, n_max=20)[0] and n <= 20 and of.shape[0] <= 1650


def test_decimate_mesh_emulated():
    check_decimate_mesh("cpu")


class Watched:
    """The library with every call of a dgs_mesh_decimate_* symbol written down."""

    def __init__(self, L):
        self._L, self.calls = L, []

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("dgs_mesh_decimate"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def check_extract_mesh(device, case, target):
    """extract_mesh(decimate_target) is decimate_mesh of what extract_mesh() returns; the default path calls none of the new symbols."""
    L = Watched(lib_of(device))
    n, r, nb, seed, sampled = FU.FIXTURE_CASES[case]
    scene, _ = FU.golden_scene(case)
    pc = FU.make_model(scene, device).apply_all_filters(**FU.PIPELINE_FILTERS)
    raw = pc.extract_mesh(FU.LEVEL, r, nb, lib=L)
    cleaned = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, min_f=8, min_d=0)
    assert pc.extract_mesh(FU.LEVEL, r, nb, lib=L, decimate_target=0).faces.shape == raw.faces.shape
    assert L.calls == []                                                      # the paths of before launch what they launched
    assert raw.faces.shape[0] > target
    mesh = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, decimate_target=target)
    assert "dgs_mesh_decimate_count" in L.calls and L.calls[-1] == "dgs_mesh_decimate_emit" and L.calls.count("dgs_mesh_decimate_emit") == 1
    dv, df, grid = decimate_mesh(raw.vertices, raw.faces, target, return_n=True, lib=L)
    assert torch.equal(mesh.vertices, dv) and torch.equal(mesh.faces, df) and mesh.vertices.device == raw.vertices.device
    assert 0 < df.shape[0] <= target
    want = D.restatement(raw.vertices.cpu().numpy(), raw.faces.cpu().numpy(), grid)
    D.assert_identical(dict(vertices=dv.cpu().numpy(), faces=df.cpu().numpy(), counts=want["counts"]), want)
    both = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, min_f=8, min_d=0, decimate_target=target)   # after the component filters
    cv, cf = decimate_mesh(cleaned.vertices, cleaned.faces, target, lib=L)
    assert torch.equal(both.vertices, cv) and torch.equal(both.faces, cf)
    small = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, decimate_target=raw.faces.shape[0])           # F <= target: the mesh as it is
    assert torch.equal(small.vertices, raw.vertices) and torch.equal(small.faces, raw.faces)
    print(case, "raw", tuple(raw.faces.shape), "target", target, "n", grid, "counts", want["counts"])


def test_extract_mesh_with_the_decimation_emulated():
    check_extract_mesh("cpu", "r32_nb8", 1500)


def test_invalid_arguments():
    """Each DGS_ERR_INVALID_ARGUMENT case returns that status and writes nothing: counts, outputs and workspace keep their fill."""
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x) for x in _tetrahedron())
    n = 8
    need = L.dgs_mesh_decimate_workspace_bytes(v.shape[0], f.shape[0], n)
    assert need > 0 and need % 16 == 0
    for V, F, k in ((-1, 5, 4), (5, -1, 4), ((1 << 30) + 1, 5, 4), (5, (1 << 30) + 1, 4), (5, 5, 0), (5, 5, 1025), (5, 5, -3)):
        assert L.dgs_mesh_decimate_workspace_bytes(V, F, k) == 0, (V, F, k)
    assert L.dgs_mesh_decimate_workspace_bytes(1 << 30, 1 << 30, 1024) > 0 and L.dgs_mesh_decimate_workspace_bytes(0, 0, 1) > 0
    assert L.dgs_mesh_decimate_workspace_bytes(100, 100, 8) <= L.dgs_mesh_decimate_workspace_bytes(100, 100, 9)        # grows with n
    ws, ws_ptr = D._guarded(need, "cpu")
    cnt, cnt_ptr = D._guarded(20, "cpu")
    ov, ov_ptr = D._guarded(12 * 4, "cpu")
    of, of_ptr = D._guarded(12 * 4, "cpu")

    def args(**over):
        a = D.make_args(L, v, f, n, ws_ptr, need, cnt_ptr)
        a.out_vertices, a.out_faces = ctypes.c_void_p(ov_ptr), ctypes.c_void_p(of_ptr)
        a.max_vertices, a.max_faces = 4, 4
        for k, x in over.items():
            setattr(a, k, x)
        return ctypes.byref(a)

    untouched = lambda: all(D._guards_intact(t, 0) for t in (ws, cnt, ov, of))
    bad = (dict(V=-1), dict(F=-1), dict(V=(1 << 30) + 1), dict(F=(1 << 30) + 1), dict(n=0), dict(n=-1), dict(n=1025), dict(vertices=None),
           dict(faces=None), dict(workspace=None), dict(workspace_bytes=need - 16), dict(workspace=ws_ptr + 8), dict(n=9))   # n = 9 needs more workspace: a second piece of the mask
    assert L.dgs_mesh_decimate_workspace_bytes(4, 4, 9) > need
    for over in bad:
        assert L.dgs_mesh_decimate_count(args(**over), None) == -1, over    # DGS_ERR_INVALID_ARGUMENT
        assert L.dgs_mesh_decimate_emit(args(**over), None) == -1, over
    assert L.dgs_mesh_decimate_count(args(counts=None), None) == -1
    assert L.dgs_mesh_decimate_count(None, None) == -1 and L.dgs_mesh_decimate_emit(None, None) == -1
    for over in (dict(out_vertices=None), dict(out_faces=None), dict(max_vertices=-1), dict(max_faces=-1)):
        assert L.dgs_mesh_decimate_emit(args(**over), None) == -1, over
    assert untouched()
    assert L.dgs_mesh_decimate_count(args(), None) == 0 and L.dgs_mesh_decimate_emit(args(), None) == 0
    assert cnt.numpy()[D.BAND:D.BAND + 20].copy().view(np.uint32).tolist() == [4, 4, 0, 0, 0]
    assert L.dgs_mesh_decimate_emit(args(out_vertices=None, max_vertices=0), None) == 0
    assert L.dgs_mesh_decimate_emit(args(out_faces=None, max_faces=0), None) == 0
    assert D._guards_intact(ws, need) and D._guards_intact(cnt, 20) and D._guards_intact(ov, 48) and D._guards_intact(of, 48)


def test_python_checks():
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x.copy()) for x in D.level_set("torus"))
    for fn, arg in ((cluster_vertices, 8), (decimate_mesh, 100)):
        for bad_v, bad_f in ((v.double(), f), (v, f.long()), (v[:, :2], f), (v, f[:, :2]), (v.reshape(-1), f), (v, f.reshape(-1))):
            with pytest.raises(ValueError):
                fn(bad_v, bad_f, arg, lib=L)
        with pytest.raises(RuntimeError, match="rebuild"):                   # a library from before the feature
            fn(v, f, arg, lib=types.SimpleNamespace())
    for n in (0, -1, 1025, 2.5):
        with pytest.raises(ValueError):
            cluster_vertices(v, f, n, lib=L)
        with pytest.raises(ValueError):
            decimate_mesh(v, f, 100, n_max=n, lib=L)
    with pytest.raises(ValueError):
        decimate_mesh(v, f, float("nan"), lib=L)
    out = cluster_vertices(v.requires_grad_(True), f, 3, lib=L)
    assert len(out) == 2 and tuple(out[0].shape) == (9, 3) and tuple(out[1].shape) == (10, 3) and not out[0].requires_grad
    assert cluster_vertices(v, f, 3, return_counts=True, lib=L)[2] == [9, 10, 2424, 6, 0]
    assert decimate_mesh(v, f, 1e5, lib=L)[1] is f                            # the reference's target: this mesh is below it


def test_abi():
    from emu_util import emu_lib
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "dgs_mesh_decimate.h")).read()
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(_native.MESH_DECIMATE_SYMBOLS) and len(names) == 3
    for lib in (emu_lib(), _native.lib()):
        for name in names:
            assert hasattr(lib, name), name
    flowed = re.sub(r"\s*\n \*\s*", " ", text)                               # the comment as running text
    assert "depends on the order in which they arrive" in flowed and "non-manifold" in flowed and "smallest input index" in flowed
    src = '#include <stdio.h>\n#include "dgs_mesh_decimate.h"\nint main(){printf("%zu\\n", sizeof(DgsMeshDecimateArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + inc, c, "-o", exe])
        assert ctypes.sizeof(_native.DgsMeshDecimateArgs) == int(subprocess.check_output([exe]))
