"""Mesh clean-up (csrc/mesh_clean.hip, include/dgs_mesh_clean.h, dgs_amd.consumers.remove_small_components, extract_mesh(min_f, min_d))
on the CPU-emulated build of the kernels: every output byte and all five counts against the numpy restatement of
tests/mesh_clean_util.py.  The checks are functions of (library, device), which tests/test_mesh_clean_gpu.py runs on the device."""
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
import mesh_clean_util as C  # noqa: E402
from dgs_amd import _native, consumers  # noqa: E402
from dgs_amd.consumers import remove_small_components  # noqa: E402  (without the feature the module fails here)

assert _native.MESH_CLEAN_SYMBOLS

# name -> (V, F, components, fewer than 64 faces, below the 20 % diagonal, surviving both): figures of a CPU probe of the fixtures
FIXTURE_STATS = {
    "noise24_08": (12911, 19446, 1269, 1228, 1262, 7),
    "noise24_05": (20016, 39161, 180, None, None, 1),
    "noise20_closed_05": (9280, 19420, 84, None, None, 1),
    "9x33x17": (6987, 13005, 54, None, None, 1),
    "sphere": (1260, 2516, 1, 0, 0, 1),
    "torus": (1220, 2440, 1, 0, 0, 1),
}
# the two rules differ on noise24 at 0.8: each alone and both
FIXTURE_RUNS = [("noise24_08", 64, 0.0), ("noise24_08", 0, 20.0), ("noise24_08", 64, 20.0), ("noise24_05", 64, 20.0),
                ("noise20_closed_05", 64, 20.0), ("9x33x17", 64, 20.0), ("sphere", 64, 20.0), ("torus", 64, 20.0), ("blobs", C.BLOB_MIN_F, 0.0),
                ("blobs", 0, C.BLOB_MIN_D), ("blobs", C.BLOB_MIN_F, C.BLOB_MIN_D)]


def lib_of(device):
    if device == "cpu":
        from emu_util import emu_lib
        return emu_lib()
    return _native.lib()


def check(device, vertices, faces, min_f, min_d, comp=None):
    """The raw call against the restatement, exactly; a second call gives the same bytes; the Python call gives the same tensors.
    -> the restatement's result."""
    L = lib_of(device)
    want = C.restatement(vertices, faces, min_f, min_d, comp)
    got = C.clean_raw(L, vertices, faces, min_f, min_d, device)
    C.assert_identical(got, want)
    C.assert_identical(C.clean_raw(L, vertices, faces, min_f, min_d, device), got)
    tv = torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device)
    tf = torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device)
    v, f, labels = remove_small_components(tv, tf, min_f=min_f, min_d=min_d, return_labels=True, lib=None if device != "cpu" else L)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and labels.dtype == torch.int32
    assert v.device == tv.device and f.device == tv.device and labels.device == tv.device and not v.requires_grad
    C.assert_identical(dict(vertices=v.cpu().numpy(), faces=f.cpu().numpy(), labels=labels.cpu().numpy(), counts=want["counts"]), want)
    return want


def test_fixture_statistics():
    """The restatement's component statistics of the marching-cubes fixtures, so that a drift of either shows."""
    for name, (V, F, ncomp, few, small, survive) in FIXTURE_STATS.items():
        v, f = C.level_set(name)
        comp = C.level_set_components(name)
        by_f, by_d = C.removed_by(comp, 64, 20.0)
        assert (v.shape[0], f.shape[0], comp["roots"].shape[0]) == (V, F, ncomp), name
        assert int((~(by_f | by_d)).sum()) == survive, name
        if few is not None:
            assert (int(by_f.sum()), int(by_d.sum())) == (few, small), name
        assert bool(comp["valid"].all()) and int(comp["n"].sum()) == F and comp["rounds"] <= 8
        assert np.array_equal(comp["roots"], np.unique(comp["labels"]))
    comp = C.level_set_components("noise24_08")
    by_f, by_d = C.removed_by(comp, 64, 20.0)
    assert bool((by_f & ~by_d).any()) or bool((by_d & ~by_f).any())          # the two rules differ here


def test_restatement_labels_are_those_of_a_sequential_union_find():
    """The propagation against forty lines of plain Python on a mesh small enough for it."""
    v, f = C.level_set("9x33x17")
    parent = list(range(v.shape[0]))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f.tolist():
        for p, q in ((a, b), (a, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    lab, _ = C.vertex_labels(v.shape[0], f)
    assert lab.tolist() == [find(x) for x in range(v.shape[0])]


def check_fixture(device, name, min_f, min_d):
    v, f = C.level_set(name)
    want = check(device, v, f, min_f, min_d, C.level_set_components(name))
    if name in ("sphere", "torus"):                                         # one component: the output is the input
        assert np.array_equal(want["vertices"].view(np.uint32), v.view(np.uint32)) and np.array_equal(want["faces"], f)
        assert want["counts"] == [v.shape[0], f.shape[0], 1, 1, 0]
    return want


@pytest.mark.parametrize("name,min_f,min_d", FIXTURE_RUNS)
def test_fixture_emulated(name, min_f, min_d):
    check_fixture("cpu", name, min_f, min_d)


def test_blob_field_each_rule_removes_what_the_other_keeps():
    comp = C.level_set_components("blobs")
    by_f, by_d = C.removed_by(comp, C.BLOB_MIN_F, C.BLOB_MIN_D)
    assert comp["roots"].shape[0] >= 6
    assert bool((by_f & ~by_d).any()) and bool((by_d & ~by_f).any()) and bool((by_f & by_d).any())
    assert int((~(by_f | by_d)).sum()) == 1 and comp["n"][~(by_f | by_d)][0] == comp["n"].max()


# ---- hand-built cases: name -> (vertices, faces, min_f, min_d) ----
def _two_tetrahedra_sharing_a_vertex():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=np.float32)
    second = np.array([0, 4, 5, 6])[np.array(C.tetrahedron(0))]
    return v, np.concatenate((np.array(C.tetrahedron(0)), second)).astype(np.int32)


def _with_unreferenced():
    v, f = C.fans([5, 70])
    pad = np.full((3, 3), 9.5, dtype=np.float32)
    v2 = np.concatenate((pad[:1], v[:4], pad[1:2], v[4:], pad[2:]))          # an unused vertex in front, one inside, one behind
    shift = np.where(f >= 4, f + 2, f + 1)
    return v2, shift.astype(np.int32)


def _with_invalid_faces():
    v, f = C.fans([5, 70, 66])
    V = v.shape[0]
    bad = np.array([[-1, 0, 1], [2, V, 3], [4, 5, 2 ** 31 - 1], [-2 ** 31, -1, V], [V, V, V]], dtype=np.int32)
    return v, np.concatenate((f[:3], bad[:2], f[3:50], bad[2:4], f[50:], bad[4:])).astype(np.int32)


def _sizes(total):
    return [total - total // 3 - 3, total // 3, 3]


def _shuffled_strip():
    return C.strip(5000, np.random.default_rng(7).permutation(5002))


HAND = {
    "one_triangle": lambda: (np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32), 64, 20.0),
    "one_triangle_kept": lambda: (np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32), 1, 100.0),
    "two_tetrahedra_one_vertex": lambda: _two_tetrahedra_sharing_a_vertex() + (8, 0.0),
    "unreferenced_vertices": lambda: _with_unreferenced() + (64, 0.0),
    "exactly_min_f": lambda: C.fans([63, 64, 65]) + (64, 0.0),
    "min_d_100_one_component": lambda: C.fans([40]) + (0, 100.0),
    "min_d_100_two_components": lambda: C.fans([40, 40]) + (0, 100.0),
    "F63": lambda: C.fans(_sizes(63)) + (4, 0.0),
    "F64": lambda: C.fans(_sizes(64)) + (4, 0.0),
    "F65": lambda: C.fans(_sizes(65)) + (4, 0.0),
    "F257": lambda: C.fans(_sizes(257)) + (4, 15.0),
    "F65600": lambda: C.fans([40000, 25000, 500, 64, 36]) + (64, 5.0),
    "strip_shuffled": lambda: _shuffled_strip() + (64, 20.0),
    "strip_descending": lambda: C.strip(5000, np.arange(5002)[::-1]) + (64, 20.0),
    "invalid_faces": lambda: _with_invalid_faces() + (66, 0.0),
    "everything_removed": lambda: C.fans([5, 6, 7]) + (64, 0.0),
}


def check_hand(device, name):
    v, f, min_f, min_d = HAND[name]()
    want = check(device, v, f, min_f, min_d)
    V, F = v.shape[0], f.shape[0]
    nv, nf, ncomp, kept, invalid = want["counts"]
    if name == "one_triangle":
        assert want["counts"] == [0, 0, 1, 0, 0]
    if name == "one_triangle_kept":
        assert want["counts"] == [3, 1, 1, 1, 0]
    if name == "two_tetrahedra_one_vertex":                                 # sharing one vertex index is enough: this pins the definition
        assert want["counts"] == [7, 8, 1, 1, 0] and bool((want["labels"] == 0).all())
    if name == "unreferenced_vertices":
        assert want["counts"] == [72, 70, 2, 1, 0] and not bool((want["vertices"] == 9.5).any())
    if name == "exactly_min_f":                                             # 63 goes; 64 and 65 stay
        assert want["counts"] == [66 + 67, 64 + 65, 3, 2, 0]
    if name == "min_d_100_one_component":                                   # d2 < D2 is false when they are equal
        assert want["counts"] == [V, F, 1, 1, 0]
    if name == "min_d_100_two_components":
        assert want["counts"] == [0, 0, 2, 0, 0]
    if name.startswith("F"):
        assert F == int(name[1:]) and ncomp == (5 if F == 65600 else 3) and 0 < kept < ncomp
    if name.startswith("strip"):                                            # deep trees: the label is the smallest index all the same
        assert want["counts"] == [V, F, 1, 1, 0] and bool((want["labels"] == 0).all())
    if name == "invalid_faces":                                             # dropped, labelled -1, counted; the neighbours as without them
        clean_v, clean_f = C.fans([5, 70, 66])
        alone = C.restatement(clean_v, clean_f, min_f, min_d)
        assert invalid == 5 and int((want["labels"] == -1).sum()) == 5
        assert want["counts"][:4] == alone["counts"][:4] and np.array_equal(want["faces"], alone["faces"])
        assert np.array_equal(want["labels"][want["labels"] >= 0], alone["labels"])
    if name == "everything_removed":
        assert want["counts"] == [0, 0, 3, 0, 0]


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_emulated(name):
    check_hand("cpu", name)


def check_empty(device):
    L = lib_of(device)
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    some_v, some_f = C.fans([5])
    for v, f, invalid in ((none_v, none_f, 0), (some_v, none_f, 0), (none_v, some_f, 5)):
        got = C.clean_raw(L, v, f, 64, 20.0, device)
        assert got["counts"] == [0, 0, 0, 0, invalid] and got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
        C.assert_identical(got, C.restatement(v, f, 64, 20.0))
        assert bool((got["labels"] == -1).all())
        out = remove_small_components(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), lib=None if device != "cpu" else L)
        assert tuple(out[0].shape) == (0, 3) and tuple(out[1].shape) == (0, 3) and out[0].dtype == torch.float32 and out[1].dtype == torch.int32


def test_empty_meshes_emulated():
    check_empty("cpu")


def check_limits(device):
    """max_vertices / max_faces below V' / F': the rows before them are the full result's; clean_raw asserts that the guard bytes behind
    them, and around the workspace and the counts, keep their fill."""
    L = lib_of(device)
    v, f = C.level_set("noise24_08")
    want = C.restatement(v, f, 64, 20.0, C.level_set_components("noise24_08"))
    nv, nf = want["counts"][:2]
    assert nv > 100 and nf > 77
    for mv, mf in ((nv, nf), (100, 77), (0, 5), (3, 0), (nv + 10, nf + 10)):
        got = C.clean_raw(L, v, f, 64, 20.0, device, max_vertices=mv, max_faces=mf, labels=mv != 3)
        assert got["counts"] == want["counts"]
        assert np.array_equal(got["vertices"].view(np.uint32), want["vertices"][:mv].view(np.uint32)) and np.array_equal(got["faces"], want["faces"][:mf])


def test_limits_leave_the_rest_untouched_emulated():
    check_limits("cpu")


def test_invalid_arguments():
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x) for x in C.fans([5, 70]))
    need = L.dgs_mesh_clean_workspace_bytes(v.shape[0], f.shape[0])
    assert need > 0 and need % 16 == 0
    for V, F in ((-1, 5), (5, -1), ((1 << 30) + 1, 5), (5, (1 << 30) + 1)):
        assert L.dgs_mesh_clean_workspace_bytes(V, F) == 0, (V, F)
    assert L.dgs_mesh_clean_workspace_bytes(1 << 30, 1 << 30) > 0 and L.dgs_mesh_clean_workspace_bytes(0, 0) > 0
    ws, counts = torch.zeros(need, dtype=torch.uint8), torch.zeros(5, dtype=torch.int32)
    out_v, out_f = torch.zeros(v.shape[0], 3), torch.zeros(f.shape[0], 3, dtype=torch.int32)

    def args(**over):
        a = C.make_args(L, v, f, 64, 20.0, ws.data_ptr(), need, counts.data_ptr())
        a.out_vertices, a.out_faces = ctypes.c_void_p(out_v.data_ptr()), ctypes.c_void_p(out_f.data_ptr())
        a.max_vertices, a.max_faces = out_v.shape[0], out_f.shape[0]
        for k, x in over.items():
            setattr(a, k, x)
        return ctypes.byref(a)

    assert L.dgs_mesh_clean_count(args(), None) == 0 and L.dgs_mesh_clean_emit(args(), None) == 0
    assert counts.tolist() == [72, 70, 2, 1, 0]
    bad = (dict(V=-1), dict(F=-1), dict(V=(1 << 30) + 1), dict(F=(1 << 30) + 1), dict(min_diag_pct=float("nan")), dict(min_diag_pct=-1.0),
           dict(min_faces=-1), dict(vertices=None), dict(faces=None), dict(workspace=None), dict(workspace_bytes=need - 16),
           dict(workspace=ws.data_ptr() + 8))
    for over in bad:
        assert L.dgs_mesh_clean_count(args(**over), None) == -1, over      # DGS_ERR_INVALID_ARGUMENT
        assert L.dgs_mesh_clean_emit(args(**over), None) == -1, over
    assert L.dgs_mesh_clean_count(args(counts=None), None) == -1
    assert L.dgs_mesh_clean_count(None, None) == -1 and L.dgs_mesh_clean_emit(None, None) == -1
    for over in (dict(out_vertices=None), dict(out_faces=None), dict(max_vertices=-1), dict(max_faces=-1)):
        assert L.dgs_mesh_clean_emit(args(**over), None) == -1, over
    assert L.dgs_mesh_clean_emit(args(out_vertices=None, max_vertices=0), None) == 0
    assert L.dgs_mesh_clean_emit(args(out_faces=None, max_faces=0), None) == 0


def test_python_checks():
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x) for x in C.fans([5, 70]))
    for bad_v, bad_f in ((v.double(), f), (v, f.long()), (v[:, :2], f), (v, f[:, :2]), (v.reshape(-1), f), (v, f.reshape(-1))):
        with pytest.raises(ValueError):
            remove_small_components(bad_v, bad_f, lib=L)
    for kw in (dict(min_f=-1), dict(min_d=-1.0), dict(min_d=float("nan")), dict(min_f=1.5)):
        with pytest.raises(ValueError):
            remove_small_components(v, f, lib=L, **kw)
    with pytest.raises(RuntimeError, match="rebuild"):                       # a library from before the feature
        remove_small_components(v, f, lib=types.SimpleNamespace())
    out = remove_small_components(v.requires_grad_(True), f, lib=L)          # the reference's values are the defaults
    assert len(out) == 2 and tuple(out[0].shape) == (72, 3) and tuple(out[1].shape) == (70, 3) and not out[0].requires_grad
    assert len(remove_small_components(v, f, return_labels=True, lib=L)) == 3
    assert tuple(remove_small_components(v, f, min_f=0, min_d=0, lib=L)[1].shape) == (75, 3)      # both rules off: only the invalid / unused go


def test_abi():
    from emu_util import emu_lib
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "dgs_mesh_clean.h")).read()
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(_native.MESH_CLEAN_SYMBOLS) and len(names) == 3
    for lib in (emu_lib(), _native.lib()):
        for n in names:
            assert hasattr(lib, n), n
    assert "depends on the order in which they arrive" in text and "closed manifold" in text      # the two sentences the header owes
    src = '#include <stdio.h>\n#include "dgs_mesh_clean.h"\nint main(){printf("%zu\\n", sizeof(DgsMeshCleanArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + inc, c, "-o", exe])
        assert ctypes.sizeof(_native.DgsMeshCleanArgs) == int(subprocess.check_output([exe]))


def check_extract_mesh(device, case):
    """extract_mesh(min_f, min_d) is remove_small_components of what extract_mesh() returns, and that is what it returned before."""
    L = None if device != "cpu" else lib_of(device)
    n, r, nb, seed, sampled = FU.FIXTURE_CASES[case]
    scene, _ = FU.golden_scene(case)
    pc = FU.make_model(scene, device).apply_all_filters(**FU.PIPELINE_FILTERS)
    raw = pc.extract_mesh(FU.LEVEL, r, nb, lib=L)
    occ = pc.extract_fields(r, nb, lib=L)
    v, t = consumers.marching_cubes(occ, FU.LEVEL, lib=L)
    assert torch.equal(raw.vertices, v / (r - 1.0) * 2 - 1) and torch.equal(raw.faces, t)          # the default: the raw level set
    comp = C.components(raw.vertices.cpu().numpy(), raw.faces.cpu().numpy())
    figures = []
    for min_f, min_d in ((64, 20), (64, 0), (0, 20)):
        mesh = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, min_f=min_f, min_d=min_d)
        cv, cf = remove_small_components(raw.vertices, raw.faces, min_f=min_f, min_d=min_d, lib=L)
        assert torch.equal(mesh.vertices, cv) and torch.equal(mesh.faces, cf) and mesh.vertices.device == raw.vertices.device
        want = C.restatement(raw.vertices.cpu().numpy(), raw.faces.cpu().numpy(), min_f, min_d, comp)
        C.assert_identical(dict(vertices=cv.cpu().numpy(), faces=cf.cpu().numpy(), counts=want["counts"]), want)
        figures.append(want["counts"])
    print(case, "V F of the raw mesh", tuple(raw.vertices.shape), tuple(raw.faces.shape), "counts", figures)
    return raw, mesh


def test_extract_mesh_with_the_clean_up_emulated():
    check_extract_mesh("cpu", "r32_nb8")


def check_ply_round_trip(device):
    v, f = C.level_set("noise20_closed_05")
    cv, cf = remove_small_components(torch.from_numpy(v.copy()).to(device), torch.from_numpy(f.copy()).to(device), lib=None if device != "cpu" else lib_of(device))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "clean.ply")
        consumers.save_mesh_ply(path, cv, cf)
        v2, f2 = consumers.load_mesh_ply(path)
    want = C.restatement(v, f, 64, 20.0, C.level_set_components("noise20_closed_05"))
    C.assert_identical(dict(vertices=v2, faces=f2, counts=want["counts"]), want)


def test_ply_round_trip_emulated():
    check_ply_round_trip("cpu")
