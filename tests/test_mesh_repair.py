"""Mesh repair (csrc/mesh_repair.hip, include/dgs_mesh_repair.h, dgs_amd.consumers.repair_mesh / mesh_topology,
extract_mesh(repair=True)) on the CPU-emulated build of the kernels: every output byte and all ten counts against the numpy restatement
of tests/mesh_repair_util.py, the census against the restated census on every input and every output.  The checks are functions of a
device, which tests/test_mesh_repair_gpu.py runs on the GPU.

Sizes.  Every kernel of csrc/mesh_repair.hip runs workgroups of 256 threads, a face, a vertex or a corner a thread; a wave is 64 rows, a
scan block 256 rows, and the one-workgroup scan over the block totals gives each of its 1,024 threads a piece of the list as long as
it has to be: there is no further stage.  So the strips have 63, 64, 65 faces (a wave), 255, 256, 257 (a workgroup and a scan block)
and 65,537 (257 scan blocks of faces, 769 of corners; the 1,024 threads of that scan take one block each up to 1,024 blocks: the
corners of 87,382 faces are the first to give a thread two, which the device test's mesh of about 10^5 faces passes).

The step-order case.  The issue asks that the census of the input show no non-manifold vertex.  No mesh on which step 3 removes
anything can do that as a whole: a face has two edges at a vertex, so the faces of a vertex joined through its edges of two faces form
paths, a face on an edge of three or more faces is an end of its path, a path has two ends, and such an edge brings three: both
vertices of every non-manifold edge are non-manifold vertices of the census.  The statement is therefore checked for the vertex that
step 3 pinches: one fan in the input, two in the restatement's intermediate."""
import collections
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
import mesh_repair_util as R  # noqa: E402
from dgs_amd import _native, consumers  # noqa: E402
from dgs_amd.consumers import repair_mesh, mesh_topology  # noqa: E402  (without the feature the module fails here)

assert _native.MESH_REPAIR_SYMBOLS and _native.MESH_REPAIR_COUNTS == R.COUNTS and _native.MESH_TOPOLOGY_COUNTS == R.TOPOLOGY


def lib_of(device):
    if device == "cpu":
        from emu_util import emu_lib
        return emu_lib()
    return _native.lib()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype.itemsize == 4 and b.dtype.itemsize == 4 and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def tensors(vertices, faces, device):
    return (torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device),
            torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device))


def check_census(device, vertices, faces):
    """dgs_mesh_topology and consumers.mesh_topology against the restated census -> the dict."""
    L = lib_of(device)
    V = int(np.shape(vertices)[0])
    want = R.census(V, faces)["numbers"]
    got = R.topology_raw(L, V, faces, device)
    assert got == want, (got, want)
    top = mesh_topology(*tensors(vertices, faces, device), lib=None if device != "cpu" else L)
    assert list(top) == list(R.TOPOLOGY) and list(top.values()) == want and all(type(x) is int for x in top.values())
    return top


def check(device, vertices, faces):
    """Everything the issue lists for a case: the raw call against the restatement, exactly; a second call gives the same bytes; the
    Python call gives the same tensors and counts; the census of the input and of the output against the restated census, and the
    output's shows no non-manifold edge and no non-manifold vertex; the faces add up; no new coordinate triangle.
    -> (the restatement's result, the census of the input)."""
    L = lib_of(device)
    want = R.restatement(vertices, faces)
    got = R.repair_raw(L, vertices, faces, device)
    print("V", np.shape(vertices)[0], "F", np.shape(faces)[0], "counts", got["counts"], "restated", want["counts"])
    R.assert_identical(got, want)
    R.assert_identical(R.repair_raw(L, vertices, faces, device), got)
    tv, tf = tensors(vertices, faces, device)
    ov, of, counts = repair_mesh(tv, tf, return_counts=True, lib=None if device != "cpu" else L)
    assert ov.dtype == torch.float32 and of.dtype == torch.int32 and ov.device == tv.device and of.device == tv.device and not ov.requires_grad
    assert list(counts) == list(R.COUNTS)
    R.assert_identical(dict(vertices=ov.cpu().numpy(), faces=of.cpu().numpy(), counts=list(counts.values())), want)
    pair = repair_mesh(tv, tf, lib=None if device != "cpu" else L)
    assert len(pair) == 2 and torch.equal(pair[0].view(torch.int32), ov.view(torch.int32)) and torch.equal(pair[1], of)
    before = check_census(device, vertices, faces)
    after = check_census(device, got["vertices"], got["faces"])
    assert after["non_manifold_edges"] == 0 and after["non_manifold_vertices"] == 0, after
    c = dict(zip(R.COUNTS, got["counts"]))
    F, V = int(np.shape(faces)[0]), int(np.shape(vertices)[0])
    assert c["faces"] == F - c["invalid_faces"] - c["null_faces"] - c["duplicate_faces"] - c["faces_removed"] == after["faces"]
    assert c["vertices"] == V - c["unreferenced_vertices"] + c["vertices_added"] == after["referenced_vertices"]
    if got["faces"].size:
        assert 0 <= int(got["faces"].min()) and int(got["faces"].max()) < c["vertices"]
        have = collections.Counter(R.triangle_multiset(vertices, np.asarray(faces)[R.valid_rows(V, faces)]))
        out = collections.Counter(R.triangle_multiset(got["vertices"], got["faces"]))
        assert not out - have                                                 # no coordinate triangle that was not there, none more often
    return want, before


# ---- the cases: name -> (vertices, faces) ----
FAR = 1.0e6
MIXED = dict(invalid_faces=4, null_faces=7, duplicate_faces=3, non_manifold_edges=0, faces_removed=0, non_manifold_vertices=1, vertices_added=2,
             unreferenced_vertices=9)


def _mixed():
    """Three tetrahedra on one vertex with unreferenced vertices in front, in the middle and at the end, and between its faces: invalid
    faces (an index of -1, of V, of 2^31 - 1, of -2^31), faces with two or three equal indices, faces without area on three distinct
    indices (two corners at one place; three on a line), a face at a NaN and one at an infinite vertex, and duplicates of faces in the
    same corner order, rotated and flipped.  The vertices that only such faces name are unreferenced too."""
    bv, bf = R.tetrahedra_on_a_vertex(3)
    pad = np.array([[FAR, -FAR, FAR]], dtype=np.float32)
    extra = np.array([bv[2], [0, 0, 0], [1, 1, 1], [2, 2, 2], [np.nan, 0.5, 0.5], [np.inf, np.inf, np.inf]], dtype=np.float32)
    v = np.concatenate((pad, bv[:5], -pad, bv[5:], extra, pad))
    f = np.where(bf < 5, bf + 1, bf + 2).astype(np.int32)
    V, e = v.shape[0], 12                                                     # e: the first row of `extra`
    invalid = [[-1, 1, 2], [2, V, 3], [4, 5, 2 ** 31 - 1], [-2 ** 31, -1, V]]
    null = [[3, 3, 5], [2, 7, 2], [4, 4, 4], [3, e, 4], [e + 1, e + 2, e + 3], [e + 4, 1, 2], [e + 5, 2, 3]]   # v[e] lies on v[3]
    dup = [list(f[1]), [f[5][1], f[5][2], f[5][0]], [f[9][0], f[9][2], f[9][1]]]
    rows = [f[:3], invalid[:2], null[:2], f[3:7], dup[:1], null[2:5], invalid[2:], f[7:], dup[1:], null[5:]]
    return v, np.concatenate([np.array(r, dtype=np.int32).reshape(-1, 3) for r in rows])


def _duplicates_first():
    """A tetrahedron whose face 0 comes three more times: flipped IN FRONT of it, then rotated and as it is behind it."""
    v, f = R.one_tetrahedron()
    a, b, c = f[0]
    return v, np.concatenate(([[a, c, b]], f, [[b, c, a]], [[a, b, c]])).astype(np.int32)


def _renamed(vertices, faces, seed):
    """Vertex i becomes perm[i]; the positions move with the names."""
    perm = np.random.default_rng(seed).permutation(vertices.shape[0])
    moved = np.empty_like(vertices)
    moved[perm] = vertices
    return moved, perm[faces].astype(np.int32)


CASES = {
    "tetrahedra_on_an_edge": R.tetrahedra_on_an_edge,
    "book_distinct": lambda: R.book("distinct"),
    "book_equal": lambda: R.book("equal"),
    "book_equal_permuted": lambda: R.book("equal", (2, 0, 1)),
    "tetrahedra_on_a_vertex": lambda: R.tetrahedra_on_a_vertex(2),
    "three_fans": lambda: R.tetrahedra_on_a_vertex(3),
    "fans_300": lambda: R.tetrahedra_on_a_vertex(300),
    "pinch_after_edges": lambda: R.pinch_after_edges()[:2],
    "tetrahedron": R.one_tetrahedron,
    "octahedron": R.octahedron,
    "voxel_ball": R.voxel_ball,
    "open_grid": lambda: R.grid(7, 5),
    "cone_16385": lambda: R.cone(16385),
    "mixed": _mixed,
    "duplicates_first": _duplicates_first,
    "strip63": lambda: R.strip(63),
    "strip64": lambda: R.strip(64),
    "strip65": lambda: R.strip(65),
    "strip255": lambda: R.strip(255),
    "strip256": lambda: R.strip(256),
    "strip257": lambda: R.strip(257),
    "strip65537": lambda: R.strip(65537),
    "fans_300_renamed": lambda: _renamed(*R.tetrahedra_on_a_vertex(300), 7),
}
UNTOUCHED = {"tetrahedron": 4, "octahedron": 8, "voxel_ball": 2512, "open_grid": 70, "cone_16385": 16385}


def check_case(device, name):
    v, f = CASES[name]()
    want, before = check(device, v, f)
    V, F = v.shape[0], f.shape[0]
    c = dict(zip(R.COUNTS, want["counts"]))
    zero = dict.fromkeys(R.COUNTS[2:], 0)
    if name == "tetrahedra_on_an_edge":                                       # four faces on {0, 1}: the two largest stay
        assert before["non_manifold_edges"] == 1 and c == dict(zero, vertices=6, faces=6, non_manifold_edges=1, faces_removed=2)
        on_edge = [i for i in range(F) if {0, 1} <= set(f[i])]
        areas = R.area2(v, f[on_edge].astype(np.int64))
        kept = sorted(np.array(on_edge)[np.argsort(areas)[2:]])
        assert [list(r) for r in want["faces"]] == [list(f[i]) for i in range(F) if i in kept or i not in on_edge]
    if name == "book_distinct":                                               # the pages reach 1, 2, 3: the first goes, and vertex 2 with it
        assert c == dict(zero, vertices=4, faces=2, non_manifold_edges=1, faces_removed=1, unreferenced_vertices=1)
        assert want["faces"].tolist() == [[1, 0, 2], [0, 1, 3]] and same_bytes(want["vertices"], v[[0, 1, 3, 4]])
    if name == "book_equal":                                                  # equal areas: the larger index goes
        assert c == dict(zero, vertices=4, faces=2, non_manifold_edges=1, faces_removed=1, unreferenced_vertices=1)
        assert want["faces"].tolist() == [[0, 1, 2], [1, 0, 3]] and same_bytes(want["vertices"], v[:4])
    if name == "book_equal_permuted":                                         # the same faces in another order: another face goes
        assert want["faces"].tolist() == [[0, 1, 3], [0, 1, 2]] and same_bytes(want["vertices"], v[[0, 1, 2, 4]])
    if name == "tetrahedra_on_a_vertex":
        assert before["non_manifold_vertices"] == 1 and c == dict(zero, vertices=8, faces=8, non_manifold_vertices=1, vertices_added=1)
        assert same_bytes(want["vertices"][:7], v) and same_bytes(want["vertices"][7], v[0])        # the copy: the same 12 bytes
        assert np.array_equal(want["faces"][:4], f[:4]) and np.array_equal(want["faces"][4:], np.where(f[4:] == 0, 7, f[4:]))
    if name == "three_fans":
        assert c == dict(zero, vertices=12, faces=12, non_manifold_vertices=1, vertices_added=2)
        assert np.array_equal(want["faces"][4:8], np.where(f[4:8] == 0, 10, f[4:8])) and np.array_equal(want["faces"][8:], np.where(f[8:] == 0, 11, f[8:]))
    if name in ("fans_300", "fans_300_renamed"):                              # more fans on one vertex than a workgroup has threads
        assert c == dict(zero, vertices=1200, faces=1200, non_manifold_vertices=1, vertices_added=299)
    if name == "fans_300_renamed":                                            # the same mesh as coordinate triangles
        base = R.restatement(*R.tetrahedra_on_a_vertex(300))
        assert R.triangle_multiset(want["vertices"], want["faces"]) == R.triangle_multiset(base["vertices"], base["faces"])
    if name == "pinch_after_edges":
        assert c == dict(zero, vertices=16, faces=8, non_manifold_edges=2, faces_removed=2, non_manifold_vertices=5, vertices_added=5)
    if name in UNTOUCHED:                                                     # the input's bytes
        assert F == UNTOUCHED[name] and c == dict(zero, vertices=V, faces=F)
        assert same_bytes(want["vertices"], v) and np.array_equal(want["faces"], f)
    if name == "mixed":
        assert c == dict(MIXED, vertices=12, faces=12)
        alone = R.restatement(*R.tetrahedra_on_a_vertex(3))                   # as without all that was mixed in
        assert same_bytes(want["vertices"], alone["vertices"]) and np.array_equal(want["faces"], alone["faces"])
    if name == "duplicates_first":                                            # the flipped face came first: it stays, flipped
        assert c == dict(zero, vertices=4, faces=4, duplicate_faces=3) and np.array_equal(want["faces"], f[[0, 2, 3, 4]])
    if name.startswith("strip"):
        assert F == int(name[5:]) and c == dict(zero, vertices=V, faces=F) and same_bytes(want["vertices"], v) and np.array_equal(want["faces"], f)


@pytest.mark.parametrize("name", list(CASES))
def test_case_emulated(name):
    check_case("cpu", name)


def test_step_order_on_the_cpu():
    """Step 3 comes before step 4: the vertex has one fan in the input and two among the faces that survive step 3 (the module's
    docstring says why the input as a whole cannot be free of non-manifold vertices)."""
    v, f, p = R.pinch_after_edges()
    V = v.shape[0]
    mid = R.restatement(v, f)["after_edges"]
    assert mid.shape[0] == f.shape[0] - 2 and [0, 1, 2] not in mid.tolist() and [0, 4, 5] not in mid.tolist()
    assert int(R.census(V, f)["fans"][p]) == 1 and int(R.census(V, mid)["fans"][p]) == 2
    assert R.census(V, mid)["numbers"][2] == 0                                # and no edge of three faces is left


def check_empty(device):
    L = lib_of(device)
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    some_v, some_f = R.strip(2)
    for v, f, counts in ((none_v, none_f, [0] * 10), (some_v, none_f, [0] * 9 + [4]), (none_v, some_f, [0, 0, 2] + [0] * 7)):
        got = R.repair_raw(L, v, f, device)
        assert got["counts"] == counts and got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
        R.assert_identical(got, R.restatement(v, f))
        ov, of, c = repair_mesh(*tensors(v, f, device), return_counts=True, lib=None if device != "cpu" else L)
        assert tuple(ov.shape) == (0, 3) and tuple(of.shape) == (0, 3) and ov.dtype == torch.float32 and of.dtype == torch.int32 and list(c.values()) == counts
        assert list(check_census(device, v, f).values()) == [0] * 7


def test_empty_meshes_emulated():
    check_empty("cpu")


SLAB_N = 12                                                                   # cells of 2 units along x; the slab is 0.3 thick


def check_slab(device):
    """What the feature is for: a thin closed slab through cluster_vertices at a cell thicker than the slab.  Where the grid's planes
    cut through it the two sheets fall into one cell here and into two there, and edges of three faces are left."""
    L = lib_of(device)
    v, f = R.slab()
    assert R.census(v.shape[0], f)["numbers"][:4] == [0, 3 * f.shape[0] // 2, 0, 0]                 # closed and manifold
    assert 24.0 / SLAB_N > 0.3
    cv, cf = consumers.cluster_vertices(*tensors(v, f, device), SLAB_N, lib=None if device != "cpu" else L)
    cv, cf = cv.cpu().numpy(), cf.cpu().numpy()
    want = D.restatement(v, f, SLAB_N)
    assert same_bytes(cv, want["vertices"]) and np.array_equal(cf, want["faces"])
    _, before = check(device, cv, cf)
    print("slab: clustered", cv.shape[0], cf.shape[0], "census", before)
    assert before["non_manifold_edges"] >= 1                                  # 12, and 16 non-manifold vertices


def test_clustered_slab_emulated():
    check_slab("cpu")


class Watched:
    """The library with every call of a symbol of include/dgs_mesh_repair.h written down."""

    def __init__(self, L):
        self._L, self.calls = L, []

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if name not in _native.MESH_REPAIR_SYMBOLS:
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def check_extract_mesh(device, case, target):
    """extract_mesh(repair=True) is repair_mesh applied by hand behind the decimation, with the smoothing and the attributes on the
    repaired mesh; the default path calls none of the new symbols and returns the bytes of the composed calls of before."""
    L = Watched(lib_of(device))
    n, r, nb, seed, sampled = FU.FIXTURE_CASES[case]
    scene, _ = FU.golden_scene(case)
    pc = FU.make_model(scene, device).apply_all_filters(**FU.PIPELINE_FILTERS)
    kw = dict(min_f=8, min_d=0, decimate_target=target)
    occ = consumers.extract_fields(pc, r, nb, lib=L)
    hv, hf = consumers.marching_cubes(occ, FU.LEVEL, lib=L)
    hv = hv / (r - 1.0) * 2 - 1
    raw = pc.extract_mesh(FU.LEVEL, r, nb, lib=L)
    assert torch.equal(raw.vertices, hv) and torch.equal(raw.faces, hf)      # the defaults: the raw level set, as ever
    hv, hf = consumers.remove_small_components(hv, hf, min_f=8, min_d=0, lib=L)
    hv, hf = consumers.decimate_mesh(hv, hf, target, lib=L)
    plain = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, **kw)
    off = consumers.extract_mesh(pc, FU.LEVEL, r, nb, lib=L, repair=False, **kw)
    assert L.calls == []                                                      # the paths of before launch what they launched
    for m in (plain, off):
        assert torch.equal(m.vertices, hv) and torch.equal(m.faces, hf) and 0 < m.faces.shape[0] <= target
    mesh = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, repair=True, **kw)
    assert L.calls == ["dgs_mesh_repair_workspace_bytes", "dgs_mesh_repair_count", "dgs_mesh_repair_emit"]
    rv, rf, counts = repair_mesh(plain.vertices, plain.faces, return_counts=True, lib=L)
    assert torch.equal(mesh.vertices, rv) and torch.equal(mesh.faces, rf) and mesh.colors is None and mesh.vertices.device == plain.vertices.device
    R.assert_identical(dict(vertices=rv.cpu().numpy(), faces=rf.cpu().numpy(), counts=list(counts.values())),
                       R.restatement(plain.vertices.cpu().numpy(), plain.faces.cpu().numpy()))
    before, after = mesh_topology(plain.vertices, plain.faces, lib=L), mesh_topology(rv, rf, lib=L)
    assert after["non_manifold_edges"] == 0 and after["non_manifold_vertices"] == 0
    full = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, repair=True, smooth_iterations=2, attributes=True, **kw)
    sv = consumers.smooth_mesh(rv, rf, 2, lib=L)                              # the smoothing and the attributes see the repaired mesh
    assert torch.equal(full.vertices, sv) and torch.equal(full.faces, rf)
    at = pc.mesh_attributes(sv, num_blocks=nb, lib=L)
    for k in ("colors", "normals", "density"):
        assert at[k].cpu().numpy().tobytes() == getattr(full, k).cpu().numpy().tobytes(), k
    print(case, "decimated", tuple(plain.faces.shape), "census", before, "counts", counts, "after", after)


def test_extract_mesh_with_the_repair_emulated():
    check_extract_mesh("cpu", "r32_nb8", 1500)


def test_invalid_arguments():
    """Each DGS_ERR_INVALID_ARGUMENT case returns that status and launches nothing: counts, outputs and workspace keep their fill."""
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x.copy()) for x in R.strip(6))
    need = L.dgs_mesh_repair_workspace_bytes(v.shape[0], f.shape[0])
    assert need > 0 and need % 16 == 0
    for V, F in ((-1, 5), (5, -1), ((1 << 30) + 1, 5), (5, (1 << 28) + 1)):
        assert L.dgs_mesh_repair_workspace_bytes(V, F) == 0, (V, F)
    assert L.dgs_mesh_repair_workspace_bytes(1 << 30, 1 << 28) > 0 and L.dgs_mesh_repair_workspace_bytes(0, 0) > 0
    ws, ws_ptr = R._guarded(need, "cpu")
    cnt, cnt_ptr = R._guarded(40, "cpu")
    top, top_ptr = R._guarded(56, "cpu")
    ov, ov_ptr = R._guarded(12 * 8, "cpu")
    of, of_ptr = R._guarded(12 * 6, "cpu")

    def args(**over):
        a = R.make_args(L, v, f, ws_ptr, need, cnt_ptr, top_ptr)
        a.out_vertices, a.out_faces, a.max_vertices, a.max_faces = ov_ptr, of_ptr, 8, 6
        for k, x in over.items():
            setattr(a, k, x)
        return ctypes.byref(a)

    sizes = (dict(V=-1), dict(F=-1), dict(V=(1 << 30) + 1), dict(F=(1 << 28) + 1), dict(faces=None), dict(workspace=None),
             dict(workspace_bytes=need - 16), dict(workspace=ws_ptr + 8), dict(V=300), dict(F=7))   # more rows need more workspace
    for fn, more in ((L.dgs_mesh_repair_count, (dict(vertices=None), dict(counts=None))), (L.dgs_mesh_topology, (dict(topology=None),)),
                     (L.dgs_mesh_repair_emit, (dict(vertices=None), dict(out_vertices=None), dict(out_faces=None), dict(max_vertices=-1), dict(max_faces=-1),
                                               dict(out_vertices=v.data_ptr()), dict(out_vertices=v.data_ptr() + 12 * 7), dict(out_vertices=v.data_ptr() - 12 * 7),
                                               dict(out_faces=f.data_ptr()), dict(out_faces=f.data_ptr() + 12 * 5), dict(out_vertices=ws_ptr + 16),
                                               dict(out_faces=ws_ptr + need - 4), dict(out_faces=ov_ptr + 12), dict(out_vertices=of_ptr - 12)))):
        for over in sizes + more:
            assert fn(args(**over), None) == -1, (fn.__name__, over)          # DGS_ERR_INVALID_ARGUMENT
        assert fn(None, None) == -1
    assert all(R._guards_intact(t, 0) for t in (ws, cnt, top, ov, of))
    fbefore, vbefore = f.numpy().copy(), v.numpy().copy()
    assert L.dgs_mesh_repair_count(args(), None) == 0 and L.dgs_mesh_repair_emit(args(), None) == 0
    assert L.dgs_mesh_repair_emit(args(counts=None, topology=None), None) == 0                       # emit needs neither
    assert cnt.numpy()[R.BAND:R.BAND + 40].copy().view(np.uint32).tolist() == [8, 6] + [0] * 8
    assert same_bytes(ov.numpy()[R.BAND:R.BAND + 96].copy().view(np.float32).reshape(8, 3), vbefore)
    assert np.array_equal(of.numpy()[R.BAND:R.BAND + 72].copy().view(np.int32).reshape(6, 3), fbefore)
    assert L.dgs_mesh_topology(args(vertices=None, counts=None), None) == 0                          # the census reads no coordinates
    assert top.numpy()[R.BAND:R.BAND + 56].copy().view(np.int64).tolist() == R.census(8, fbefore)["numbers"]
    assert all(R._guards_intact(t, n) for t, n in ((ws, need), (cnt, 40), (top, 56), (ov, 96), (of, 72)))
    assert np.array_equal(v.numpy(), vbefore) and np.array_equal(f.numpy(), fbefore)
    fresh_v, fresh_f = R._guarded(96, "cpu"), R._guarded(72, "cpu")                                  # fewer rows than the result has: nothing beyond them
    assert L.dgs_mesh_repair_emit(args(out_vertices=fresh_v[1], out_faces=fresh_f[1], max_vertices=3, max_faces=2), None) == 0
    assert R._guards_intact(fresh_v[0], 36) and R._guards_intact(fresh_f[0], 24)
    assert np.array_equal(fresh_f[0].numpy()[R.BAND:R.BAND + 24].copy().view(np.int32).reshape(2, 3), fbefore[:2])


def test_python_checks():
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x.copy()) for x in R.tetrahedra_on_a_vertex(2))
    for fn in (repair_mesh, mesh_topology):
        for bad_v, bad_f in ((v.double(), f), (v, f.long()), (v[:, :2], f), (v, f[:, :2]), (v.reshape(-1), f), (v, f.reshape(-1))):
            with pytest.raises(ValueError):
                fn(bad_v, bad_f, lib=L)
        with pytest.raises(RuntimeError, match="rebuild"):                   # a library from before the feature
            fn(v, f, lib=types.SimpleNamespace())
    ov, of = repair_mesh(v.clone().requires_grad_(True), f, lib=L)
    assert tuple(ov.shape) == (8, 3) and tuple(of.shape) == (8, 3) and not ov.requires_grad
    strided = torch.zeros((v.shape[0], 6))[:, ::2]                            # not contiguous: taken as it reads
    strided.copy_(v)
    sv, sf = repair_mesh(strided, f, lib=L)
    assert torch.equal(sv, ov) and torch.equal(sf, of)
    assert mesh_topology(v, f, lib=L)["non_manifold_vertices"] == 1 and mesh_topology(ov, of, lib=L)["non_manifold_vertices"] == 0


def test_abi():
    from emu_util import emu_lib
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "dgs_mesh_repair.h")).read()
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(_native.MESH_REPAIR_SYMBOLS) and len(names) == 4
    for lib in (emu_lib(), _native.lib()):
        for name in names:
            assert hasattr(lib, name), name
    flowed = re.sub(r"\s*\n \*\s*", " ", text)                               # the comment as running text
    for phrase in ("The same input gives the same bytes in every run", "Renaming the vertices", "Permuting the faces can change the tie-breaks",
                   "Orientation is neither checked nor repaired", "it becomes a border edge of the output", "comes back byte for byte",
                   "V in [0, 2^30]", "F in [0, 2^28]"):
        assert phrase in flowed, phrase
    assert int(re.search(r"#define DGS_MESH_REPAIR_COUNTS (\d+)", text).group(1)) == len(R.COUNTS)
    assert int(re.search(r"#define DGS_MESH_TOPOLOGY_COUNTS (\d+)", text).group(1)) == len(R.TOPOLOGY)
    src = '#include <stdio.h>\n#include "dgs_mesh_repair.h"\nint main(){printf("%zu\\n", sizeof(DgsMeshRepairArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + inc, c, "-o", exe])
        assert ctypes.sizeof(_native.DgsMeshRepairArgs) == int(subprocess.check_output([exe]))
    smooth = open(os.path.join(inc, "dgs_mesh_smooth.h")).read()
    assert "dgs_mesh_repair.h" in smooth                                     # its "what this is not" points to the new call
