"""Marching cubes (csrc/mesh.hip, tools/make_mc_table.py, dgs_amd.consumers.marching_cubes / save_mesh_ply, GaussianModel.extract_mesh)
on the CPU-emulated build of the kernels: bit for bit against the sequential restatement of tests/mesh_util.py, and against the checks
there that do not trust the table."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import field_util as FU  # noqa: E402
import mesh_util as U  # noqa: E402

# name -> (occ, level, expected figures or None)
NAMED = {
    "sphere": lambda: (U.sphere(), 0.0, dict(V=1260, F=2516, open=0, euler=2)),
    "torus": lambda: (U.torus(), 0.0, dict(V=1220, F=2440, open=0, euler=0)),
    "noise24": lambda: (U.noise_pair()[0], 0.5, dict(V=20016, F=39161, open=3205)),
    "noise20_closed": lambda: (U.noise_pair()[1], 0.5, dict(V=9280, F=19420, open=0)),
    "one_cell": lambda: (U.shaped_noise((2, 2, 2), 3), 0.5, None),
    "row_of_three_words": lambda: (U.shaped_noise((2, 2, 130), 4), 0.5, None),
    "5x70x9": lambda: (U.shaped_noise((5, 70, 9), 5), 0.5, None),
    "65x3x64": lambda: (U.shaped_noise((65, 3, 64), 6), 0.5, None),
    "64x3x65": lambda: (U.shaped_noise((64, 3, 65), 7), 0.5, None),
    "max_faces_only": lambda: (U.max_face_only(), 0.5, None),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (occ, level, expected, restatement's vertices, triangles, check_mesh of them): computed once, shared, never modified."""
    occ, level, expected = NAMED[name]()
    v, t = U.restatement(occ, level)
    return occ, level, expected, v, t, U.check_mesh(occ, level, v, t)


def run(occ, level, lib, device):
    from dgs_amd import consumers
    v, t = consumers.marching_cubes(torch.from_numpy(np.ascontiguousarray(occ)).to(device), level, lib=lib)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.device.type == torch.device(device).type
    assert v.dim() == 2 and v.shape[1] == 3 and t.dim() == 2 and t.shape[1] == 3
    return v.cpu().numpy(), t.cpu().numpy()


def check_named_case(name, lib, device):
    """Bitwise vertices, equal triangles, the table-independent checks on the product's own output, two calls the same bits."""
    occ, level, expected, rv, rt, rfig = reference(name)
    v, t = run(occ, level, lib, device)
    assert v.shape == rv.shape and t.shape == rt.shape, (v.shape, rv.shape, t.shape, rt.shape)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)), int((v.view(np.uint32) != rv.view(np.uint32)).sum())
    assert np.array_equal(t, rt)
    fig = U.check_mesh(occ, level, v, t)
    print(name, fig)
    assert fig == rfig
    if expected:
        assert fig["V"] == expected["V"] and fig["F"] == expected["F"] and fig["open"] == expected["open"]
        if "euler" in expected:
            assert fig["V"] - fig["E"] + fig["F"] == expected["euler"]
    v2, t2 = run(occ, level, lib, device)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(t2, t)
    return fig


def test_table_is_the_generators_and_has_the_stated_size():
    import make_mc_table
    assert open(make_mc_table.HEADER).read() == make_mc_table.header_text()
    t = make_mc_table.table()
    assert len(t) == 256 and max(len(x) for x in t) == 5 and sum(len(x) for x in t) == 820
    assert t[0] == [] and t[255] == []
    used = [set(e for tri in tris for e in tri) for tris in t]
    assert all(used[c] == used[255 - c] for c in range(256))
    words = make_mc_table.packed(t)
    text = open(make_mc_table.HEADER).read()
    assert [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", text)] == words
    for c, tris in enumerate(t):                                            # every loop's polygon: n edges -> n - 2 triangles
        assert len(tris) == sum(len(loop) - 2 for loop in make_mc_table.loops(c))
        for loop in make_mc_table.loops(c):
            assert 3 <= len(loop) <= 12


def test_restatement_volumes_and_case_coverage():
    """The chord error of the method: the restatement's signed volume within 2 % of the analytic one, and positive (the winding)."""
    _, _, _, v, t, _ = reference("sphere")
    vol, exact = U.signed_volume(v, t), 4.0 / 3.0 * math.pi * U.SPHERE_RADIUS ** 3
    print(f"sphere: volume {vol:.2f} against {exact:.2f} ({(vol / exact - 1) * 100:+.2f} %)")
    assert abs(vol / exact - 1) < 0.02
    _, _, _, v, t, _ = reference("torus")
    vol, exact = U.signed_volume(v, t), 2.0 * math.pi ** 2 * U.TORUS_MAJOR * U.TORUS_MINOR ** 2
    print(f"torus: volume {vol:.2f} against {exact:.2f} ({(vol / exact - 1) * 100:+.2f} %)")
    # an inscribed polygon with chords of length l loses l^2 / (6 r^2) of a circle's area; mesh edges are at most a cell's diagonal,
    # l^2 <= 3, and the torus curves with 1 / r of the tube and at most 1 / (R - r) around the axis
    assert 0 < vol < exact and 1 - vol / exact < 3 / (6 * U.TORUS_MINOR ** 2) + 3 / (6 * (U.TORUS_MAJOR - U.TORUS_MINOR) ** 2)
    for name in ("noise24", "noise20_closed"):
        occ, level = reference(name)[:2]
        assert np.unique(U.cases(occ, level)).shape[0] == 256, name


@pytest.mark.parametrize("name", list(NAMED))
def test_mesh_matches_the_restatement_emulated(name):
    from emu_util import emu_lib
    check_named_case(name, emu_lib(), "cpu")


def test_no_crossing_gives_empty_tensors():
    from emu_util import emu_lib
    for occ in (np.zeros((4, 3, 5), dtype=np.float32), np.ones((4, 3, 5), dtype=np.float32)):
        v, t = run(occ, 0.5, emu_lib(), "cpu")
        assert v.shape == (0, 3) and t.shape == (0, 3)
        rv, rt = U.restatement(occ, 0.5)
        assert rv.shape == (0, 3) and rt.shape == (0, 3)


def test_equality_is_outside_and_nan_is_outside():
    """occ == level is outside (t = 0: the vertex sits on the sample); a NaN sample is outside like any other."""
    from emu_util import emu_lib
    occ = np.zeros((3, 3, 3), dtype=np.float32)
    occ[1, 1, 1] = 1.0
    v, t = run(occ, 0.0, emu_lib(), "cpu")                                 # every neighbour equals the level
    rv, rt = U.restatement(occ, 0.0)
    assert v.shape == (6, 3) and t.shape == (8, 3) and np.array_equal(v, rv) and np.array_equal(t, rt)
    assert sorted(map(tuple, v.tolist())) == sorted([(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)])
    v, t = run(1.0 - occ, 1.0, emu_lib(), "cpu")                           # everything equals the level or is below it
    assert v.shape == (0, 3) and t.shape == (0, 3)
    occ[0, 0, 0] = np.nan
    v, t = run(occ, 0.5, emu_lib(), "cpu")
    assert v.shape == (6, 3) and t.shape == (8, 3) and bool(np.isfinite(v).all())


def _call_args(L, occ, level, ws, counts, vertices=None, triangles=None, /, **over):
    from dgs_amd import _native
    a = _native.DgsMeshArgs()
    a.X, a.Y, a.Z = occ.shape
    a.level = level
    a.workspace_bytes = ws.numel()
    a.occ, a.counts, a.workspace = (ctypes.c_void_p(t.data_ptr()) for t in (occ, counts, ws))
    if vertices is not None:
        a.vertices, a.triangles = ctypes.c_void_p(vertices.data_ptr()), ctypes.c_void_p(triangles.data_ptr())
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_guards():
    from emu_util import emu_lib
    L = emu_lib()
    occ = torch.from_numpy(U.shaped_noise((6, 5, 7), 9))
    need = L.dgs_marching_cubes_workspace_bytes(6, 5, 7)
    assert need > 0 and need % 16 == 0
    for shape in ((1, 5, 7), (6, 1, 7), (6, 5, 1), (1024, 1024, 1025), (0, 0, 0)):
        assert L.dgs_marching_cubes_workspace_bytes(*shape) == 0, shape
    assert L.dgs_marching_cubes_workspace_bytes(1024, 1024, 1024) > 0       # 2^30 samples: the largest grid
    ws, counts = torch.zeros(need, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32)
    vertices, triangles = torch.zeros(2000, 3), torch.zeros(4000, 3, dtype=torch.int32)

    def count(**over):
        return L.dgs_marching_cubes_count(ctypes.byref(_call_args(L, occ, 0.5, ws, counts, **over)), None)

    def emit(**over):
        a = _call_args(L, occ, 0.5, ws, counts, vertices, triangles, **{**dict(max_vertices=2000, max_triangles=4000), **over})
        return L.dgs_marching_cubes_emit(ctypes.byref(a), None)

    assert count() == 0 and emit() == 0
    bad = (dict(X=1), dict(Y=1), dict(Z=1), dict(X=1 << 20, Y=1 << 10, Z=2), dict(level=float("nan")), dict(occ=None), dict(workspace=None),
           dict(workspace_bytes=need - 16), dict(workspace=ws.data_ptr() + 8))
    for over in bad:
        assert count(**over) == -1, over                                    # DGS_ERR_INVALID_ARGUMENT
        assert emit(**over) == -1, over
    assert count(counts=None) == -1
    for over in (dict(vertices=None), dict(triangles=None), dict(max_vertices=-1), dict(max_triangles=-1)):
        assert emit(**over) == -1, over
    assert emit(vertices=None, max_vertices=0) == 0 and emit(triangles=None, max_triangles=0) == 0
    with pytest.raises(ValueError):
        from dgs_amd import consumers
        consumers.marching_cubes(torch.zeros(1, 4, 4), 0.5, lib=L)
    with pytest.raises(ValueError):
        consumers.marching_cubes(torch.zeros(4, 4, 4, dtype=torch.float64), 0.5, lib=L)


def check_limits(lib, device):
    """max_vertices / max_triangles below V / F: the rows before them are the full result's, everything after them (guard bands
    included) keeps its fill."""
    occ_np, level, _, rv, rt, _ = reference("noise20_closed")
    occ = torch.from_numpy(occ_np).to(device)
    L = lib
    ws = torch.zeros(L.dgs_marching_cubes_workspace_bytes(*occ.shape), dtype=torch.uint8, device=device)
    counts = torch.zeros(2, dtype=torch.int32, device=device)
    assert L.dgs_marching_cubes_count(ctypes.byref(_call_args(L, occ, level, ws, counts)), None) == 0
    assert counts.tolist() == [rv.shape[0], rt.shape[0]]
    for mv, mt in ((rv.shape[0], rt.shape[0]), (1000, 777), (0, 5), (3, 0)):
        band = 64
        vbuf = torch.full((rv.shape[0] + 2 * band, 3), -7.0, device=device)
        tbuf = torch.full((rt.shape[0] + 2 * band, 3), -7, dtype=torch.int32, device=device)
        a = _call_args(L, occ, level, ws, counts, vbuf[band:], tbuf[band:], max_vertices=mv, max_triangles=mt)
        assert L.dgs_marching_cubes_emit(ctypes.byref(a), None) == 0
        if device != "cpu":
            torch.cuda.synchronize()
        v, t = vbuf.cpu().numpy(), tbuf.cpu().numpy()
        assert np.array_equal(v[band:band + mv], rv[:mv]) and np.array_equal(t[band:band + mt], rt[:mt])
        assert bool((v[:band] == -7).all()) and bool((v[band + mv:] == -7).all())
        assert bool((t[:band] == -7).all()) and bool((t[band + mt:] == -7).all())


def test_limits_leave_the_rest_untouched_emulated():
    from emu_util import emu_lib
    check_limits(emu_lib(), "cpu")


def test_abi():
    from dgs_amd import _native
    from emu_util import emu_lib
    inc = os.path.join(ROOT, "include")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgs_mesh.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_native.MESH_SYMBOLS) and len(names) == 3
    for lib in (emu_lib(), _native.lib()):
        for n in names:
            assert hasattr(lib, n), n
    src = '#include <stdio.h>\n#include "dgs_mesh.h"\nint main(){printf("%zu\\n", sizeof(DgsMeshArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + inc, c, "-o", exe])
        assert ctypes.sizeof(_native.DgsMeshArgs) == int(subprocess.check_output([exe]))


def check_pipeline_case(name, lib, device):
    """apply_all_filters -> extract_mesh on a fixture scene: the restatement applied to extract_fields' own output, normalised with the
    same fp32 expression; vertices within [-1, 1]; mesh_center / mesh_scale as extract_fields sets them."""
    n, r, nb, seed, sampled = FU.FIXTURE_CASES[name]
    scene, _ = FU.golden_scene(name)
    pc = FU.make_model(scene, device).apply_all_filters(**FU.PIPELINE_FILTERS)
    mesh = pc.extract_mesh(FU.LEVEL, r, nb, lib=lib)
    center, scale = pc.mesh_center.clone(), pc.mesh_scale
    occ = pc.extract_fields(r, nb, lib=lib)
    assert torch.equal(pc.mesh_center, center) and pc.mesh_scale == scale
    rv, rt = U.restatement(occ.cpu().numpy(), FU.LEVEL)
    assert rv.shape[0] > 100 and rt.shape[0] > 100
    want = (torch.from_numpy(rv).to(device) / (r - 1.0) * 2 - 1).cpu()       # the same torch expression on the same device
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and mesh.vertices.device == occ.device
    assert torch.equal(mesh.vertices.cpu(), want) and np.array_equal(mesh.faces.cpu().numpy(), rt)
    assert float(mesh.vertices.min()) >= -1.0 and float(mesh.vertices.max()) <= 1.0
    assert not bool((occ == np.float32(FU.LEVEL)).any())
    fig = U.check_mesh(occ.cpu().numpy(), FU.LEVEL, rv, rt, strict_inside=False)
    print(name, fig)
    return mesh


def test_extract_mesh_on_a_fixture_scene_emulated():
    from emu_util import emu_lib
    mesh = check_pipeline_case("r32_nb8", emu_lib(), "cpu")
    assert "Mesh(vertices=" in repr(mesh)


def test_mesh_ply_round_trip():
    from dgs_amd import consumers
    _, _, _, v, t, _ = reference("torus")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sub", "mesh.ply")
        consumers.save_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(t))
        raw = open(path, "rb").read()
        head = ("ply\nformat binary_little_endian 1.0\nelement vertex 1220\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 2440\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
        assert raw.startswith(head) and len(raw) == len(head) + 12 * 1220 + 13 * 2440
        v2, t2 = consumers.load_mesh_ply(path)
        assert v2.dtype == np.float32 and t2.dtype == np.int32
        assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(t2, t)
        consumers.save_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))      # an empty mesh is a valid file
        v3, t3 = consumers.load_mesh_ply(path)
        assert v3.shape == (0, 3) and t3.shape == (0, 3)
