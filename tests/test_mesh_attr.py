"""Mesh attributes (csrc/mesh_attr.hip, include/dgs_mesh_attr.h, dgs_amd.consumers.mesh_attributes, extract_mesh(attributes=True),
save_mesh_ply / load_mesh_ply with colours and normals) on the CPU-emulated build of the kernels, against the fp64 restatement and the
bars of tests/mesh_attr_util.py.  The checks are functions of a device, which tests/test_mesh_attr_gpu.py runs on the GPU.

Sizes.  The evaluation kernel runs workgroups of 256 threads, lane = point, and stages 256 records at a time; a workgroup owns 4
z-adjacent point cells.  So: 63 / 65 / 257 points, a cell of 300 Gaussians (two stages), a row of 600 (three), 300 points in one cell
(two passes), grids of 1, 4, 5 and 8 cells per axis (5: a last run of one cell), reach 0, 1, 2 and beyond the grid."""
import ctypes
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

import field_util as FU  # noqa: E402
import mesh_attr_util as M  # noqa: E402
from dgs_amd import _native, consumers  # noqa: E402
from dgs_amd.consumers import mesh_attributes  # noqa: E402  (without the feature the module fails here)

assert _native.MESH_ATTR_SYMBOLS

REPORT = []                    # the printed err / bar lines, for tools/mesh_attr_error.py


def lib_of(device):
    if device == "cpu":
        from emu_util import emu_lib
        return emu_lib()
    return _native.lib()


def py_lib(device):
    return lib_of(device) if device == "cpu" else None


def run_case(device, name, g, attr, points, nb, reach, level_set=False):
    """raw call vs restatement under the bars; a second call gives the same bytes.  -> (outputs, ref64)"""
    L = lib_of(device)
    ref = M.restate(g, attr, points, nb, reach, device=device)
    e32 = M.e32_of(g, attr, points, nb, reach, ref, device=device)
    rc, got, whole = M.raw(L, device, g, attr, points, nb, reach)
    assert rc == 0
    M.check_case(f"{name} [{device}]", got, ref, e32, attr, level_set, REPORT)
    rc2, _, whole2 = M.raw(L, device, g, attr, points, nb, reach)
    assert rc2 == 0 and all(whole[k].tobytes() == whole2[k].tobytes() for k in whole)
    return got, ref


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---- trivial sizes and single-Gaussian geometry ----
def check_trivial(device):
    L = lib_of(device)
    one = dict(xyz=torch.tensor([[0.1, -0.2, 0.3]]), scaling=torch.full((1, 3), float(np.log(0.2))), rotation=torch.tensor([[1.0, 0.2, -0.1, 0.3]]),
               opacity=torch.tensor([0.5]), mesh_scale=1.0, scaling_modifier=1.0)
    attr1 = torch.tensor([[0.25, 0.5, 0.75]])
    got, ref = run_case(device, "N1_V1", one, attr1, torch.tensor([[0.2, -0.1, 0.2]]), 4, 1)
    assert ref["n"].tolist() == [1] and got["density"][0] > 0.1
    rc, got, whole = M.raw(L, device, one, attr1, torch.zeros(0, 3), 4, 1)                       # V = 0: DGS_OK, nothing launched
    assert rc == 0 and all((b == M.SENTINEL).all() for b in whole.values())
    g, attr = M.random_scene(300, 11)
    for v in (63, 65, 257):
        run_case(device, f"V{v}", g, attr, M.random_points(v, v), 4, 1)


def sphere_case():
    """One isotropic Gaussian at the origin (s = 0.1) and two helpers in the far corners that make the normalisation the identity
    (centre 0, scale 1) and lie outside every point's window; 200 points on the sphere of radius 0.15."""
    scene = dict(xyz=torch.tensor([[0.0, 0.0, 0.0], [-0.9, -0.9, -0.9], [0.9, 0.9, 0.9]]), scaling=torch.full((3, 3), float(np.log(0.1))),
                 rotation=torch.tensor([[1.0, 0, 0, 0]] * 3), opacity=torch.tensor([[1.0], [0.0], [0.0]]),
                 features=torch.tensor([[[0.9, -0.4, 0.3]], [[1.0, 1.0, 1.0]], [[-1.0, -1.0, -1.0]]]))
    q = torch.Generator().manual_seed(5)
    d = torch.rand(200, 3, generator=q, dtype=torch.float64) * 2 - 1
    d = d / torch.sqrt((d * d).sum(1, keepdim=True))
    return scene, (0.15 * d).float()


def check_sphere(device):
    scene, points = sphere_case()
    g, attr = M.scene_inputs(scene)
    assert float(np.float32(g["mesh_scale"])) == 1.0 and bool((g["xyz"] == scene["xyz"]).all())
    got, ref = run_case(device, "sphere", g, attr, points, 8, 1)
    assert ref["n"].tolist() == [1] * 200
    r2 = (points.double() ** 2).sum(1)
    s = float(np.exp(np.float64(np.float32(np.log(0.1)))))                                       # the stored log scale is fp32
    closed = torch.sigmoid(torch.tensor(1.0, dtype=torch.float64)) * torch.exp(-0.5 * r2 / s ** 2)
    assert float((ref["density"] - closed).abs().max()) <= 1e-12                                  # the restatement against the closed form
    assert float((torch.from_numpy(got["density"].copy()).double() - closed).abs().max()) <= 4 * 2.0 ** -24 * float(closed.max())
    assert float((torch.from_numpy(got["attr"].copy()) - attr[0][None]).abs().max()) <= 2 * 2.0 ** -24
    out = mesh_attributes(FU.make_model(scene, device), points.to(device), num_blocks=8, reach=1, lib=py_lib(device))
    radial = points.double() / torch.sqrt(r2)[:, None]
    assert float((out["normals"].cpu().double() - radial).abs().max()) <= 1e-5
    assert out["colors"].cpu().numpy().tobytes() == got["attr"].tobytes() and out["density"].cpu().numpy().tobytes() == got["density"].tobytes()


def blobs_scene():
    """Three blobs of radius ~0.38 at the level 0.005, apart from each other and inside the cube; two invisible helpers (opacity logit
    -20) in the corners make the normalisation the identity."""
    return dict(xyz=torch.tensor([[-0.5, -0.4, -0.45], [0.5, -0.3, 0.4], [0.0, 0.5, 0.0], [-0.9, -0.9, -0.9], [0.9, 0.9, 0.9]]),
                scaling=torch.full((5, 3), float(np.log(0.12))), rotation=torch.tensor([[1.0, 0, 0, 0]] * 5),
                opacity=torch.tensor([[2.0], [1.0], [3.0], [-20.0], [-20.0]]),
                features=torch.tensor([[[1.5, -1.0, 0.0]], [[0.0, 1.0, -1.5]], [[-1.0, 0.2, 1.2]], [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]]]))


def vertex_face_agreement(vertices, faces, normals):
    """Smallest dot product of a vertex normal with the mean normal of its adjacent faces (fp64)."""
    v, f = vertices.double(), faces.long()
    fn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    fn = fn / torch.sqrt((fn * fn).sum(1, keepdim=True)).clamp_min(1e-300)
    mean = torch.zeros_like(v)
    for k in range(3):
        mean.index_add_(0, f[:, k], fn)
    return float((mean * normals.double()).sum(1).min())


def check_blobs(device):
    """Three separated isotropic Gaussians meshed at R = 32: the gradient normals agree with the faces' winding."""
    scene = blobs_scene()
    pc = FU.make_model(scene, device)
    mesh = consumers.extract_mesh(pc, resolution=32, num_blocks=8, lib=py_lib(device), attributes=True)
    assert mesh.faces.shape[0] > 100
    g, attr = M.scene_inputs(scene)
    ref = M.restate(g, attr, mesh.vertices.cpu(), 8, 2)
    rn = -ref["grad"] / torch.sqrt((ref["grad"] ** 2).sum(1, keepdim=True))
    assert vertex_face_agreement(mesh.vertices.cpu(), mesh.faces.cpu(), rn) > 0                   # on the restatement first
    assert vertex_face_agreement(mesh.vertices.cpu(), mesh.faces.cpu(), mesh.normals.cpu()) > 0
    assert float((mesh.normals.cpu().double() - rn).abs().max()) <= 1e-4


# ---- staging and binning limits ----
def crowded_case():
    """nb = 5, reach = 1.  Cell (2, 2, 2) holds 300 Gaussians (two LDS stages); row (1, 3, *) holds 600 over its five cells; 300 points
    lie in cell (2, 2, 2) (two passes), 40 in row (1, 3, *), 24 spread wide; most point cells are empty."""
    q = torch.Generator().manual_seed(21)
    r = lambda *s: torch.rand(*s, generator=q, dtype=torch.float64)
    pitch = 0.4
    lo = lambda c: -1 + pitch * c
    a = torch.stack([lo(2) + pitch * (0.02 + 0.96 * r(300)) for _ in range(3)], 1)
    b = torch.stack([lo(1) + pitch * (0.02 + 0.96 * r(600)), lo(3) + pitch * (0.02 + 0.96 * r(600)), -0.98 + 1.96 * r(600)], 1)
    c = (2 * r(100, 3) - 1) * 0.95
    xyz = torch.cat((a, b, c)).float()
    n = xyz.shape[0]
    g = dict(xyz=xyz, scaling=(np.log(0.05) + (np.log(0.25) - np.log(0.05)) * r(n, 3)).float(), rotation=(2 * r(n, 4) - 0.9).float(),
             opacity=(4 * r(n) - 2).float(), mesh_scale=1.0, scaling_modifier=1.0)
    pa = torch.stack([lo(2) + pitch * (0.02 + 0.96 * r(300)) for _ in range(3)], 1)
    pb = torch.stack([lo(1) + pitch * (0.02 + 0.96 * r(40)), lo(3) + pitch * (0.02 + 0.96 * r(40)), -0.98 + 1.96 * r(40)], 1)
    pts = torch.cat((pa, pb, (2 * r(24, 3) - 1) * 0.95)).float()
    return g, r(n, 3).float(), pts


def check_crowded(device):
    g, attr, pts = crowded_case()
    gc = M.cell(g["xyz"], 5)
    key = (gc[:, 0] * 5 + gc[:, 1]) * 5 + gc[:, 2]
    counts = torch.bincount(key, minlength=125)
    assert int(counts[(2 * 5 + 2) * 5 + 2]) > 256 and int(counts.reshape(5, 5, 5)[1, 3].sum()) > 512
    pc = M.cell(pts, 5)
    pcount = torch.bincount((pc[:, 0] * 5 + pc[:, 1]) * 5 + pc[:, 2], minlength=125)
    assert int(pcount.max()) > 256 and int((pcount == 0).sum()) > 60
    run_case(device, "crowded", g, attr, pts, 5, 1)


# ---- window edges and bad input ----
def edge_points(nb):
    ks = torch.arange(nb + 1, dtype=torch.float64)
    b = (-1 + ks * 2 / nb).float()
    axis = torch.cat((b, torch.tensor([-1.3, 1.3, 0.05])))
    q = torch.Generator().manual_seed(3)
    pick = lambda: axis[torch.randint(0, axis.numel(), (120,), generator=q)]
    pts = torch.stack((pick(), pick(), pick()), 1)
    corners = torch.tensor([[-1.0, -1, -1], [1, 1, 1], [-1.3, 1.3, 0.0], [1.3, -1.3, 1.3], [-1, 1, -1.3]])
    return torch.cat((corners, pts))


def check_edges(device):
    L = lib_of(device)
    g, attr = M.random_scene(400, 31, spread=1.0)
    for nb, reach in ((8, 2), (1, 0), (4, 0), (3, 3), (2, 8)):
        pts = edge_points(max(nb, 2))
        got, ref = run_case(device, f"edges_nb{nb}_reach{reach}", g, attr, pts, nb, reach)
        if reach >= nb:
            assert bool((ref["n"] == 400).all())                                                   # the window is the whole grid
    # a NaN point among good ones: rc 0, the good ones keep their bits
    pts = edge_points(8)
    bad = torch.cat((pts[:50], torch.tensor([[float("nan"), 0.1, 0.2], [0.3, float("nan"), float("nan")]]), pts[50:]))
    rc, clean, _ = M.raw(L, device, g, attr, pts, 8, 2)
    rc2, dirty, _ = M.raw(L, device, g, attr, bad, 8, 2)
    keep = [i for i in range(bad.shape[0]) if i not in (50, 51)]
    assert rc == 0 and rc2 == 0 and all(clean[k].tobytes() == dirty[k][keep].tobytes() for k in clean)
    # an empty window: exactly 0 everywhere.  Gaussians only in the -x half, points in the +x corner, reach 1 of 8 cells
    far = dict(g, xyz=g["xyz"] * torch.tensor([0.4, 1, 1]) - torch.tensor([0.5, 0, 0]))
    corner = torch.tensor([[0.9, 0.9, 0.9], [0.8, -0.9, 0.1], [1.3, 0.0, 0.0]])
    rc, got, _ = M.raw(L, device, far, attr, corner, 8, 1)
    assert rc == 0 and bool((M.restate(far, attr, corner, 8, 1)["n"] == 0).all()) and all((got[k] == 0).all() for k in got)
    # every term underflows: a narrow Gaussian (s = 0.002) one cell away -> power far below -126, the weight flushes to 0
    narrow = dict(xyz=torch.tensor([[0.0, 0.0, 0.0]]), scaling=torch.full((1, 3), float(np.log(0.002))), rotation=torch.tensor([[1.0, 0, 0, 0]]),
                  opacity=torch.tensor([3.0]), mesh_scale=1.0, scaling_modifier=1.0)
    rc, got, _ = M.raw(L, device, narrow, torch.tensor([[0.3, 0.6, 0.9]]), torch.tensor([[0.2, 0.1, 0.1], [-0.2, 0.05, 0.0]]), 8, 2)
    ref = M.restate(narrow, torch.tensor([[0.3, 0.6, 0.9]]), torch.tensor([[0.2, 0.1, 0.1], [-0.2, 0.05, 0.0]]), 8, 2)
    assert rc == 0 and ref["n"].tolist() == [1, 1] and bool((ref["density"] < 2.0 ** -150).all())
    assert (got["attr"] == 0).all() and (got["density"] == 0).all() and np.isfinite(got["grad"]).all()


# ---- fixture scenes and the pipeline path ----
_meshes = {}


def fixture_mesh(name, filtered, device):
    """The vertices extract_mesh gives at the scene's R and nb (filtered: after min_f=64, min_d=20 and a decimation target)."""
    key = (name, filtered, device)
    if key not in _meshes:
        n, r, nb, seed, _ = FU.FIXTURE_CASES[name]
        scene = FU.golden_scene(name)[1]                                         # regenerated from its seed, after the pipeline's filters
        pc = FU.make_model(scene, device)
        kw = dict(min_f=64, min_d=20, decimate_target=1500) if filtered else {}
        mesh = consumers.extract_mesh(pc, resolution=r, num_blocks=nb, lib=py_lib(device), **kw)
        _meshes[key] = (scene, mesh)
    return _meshes[key]


def check_fixture(device, name, filtered, stride=1):
    n, r, nb, seed, _ = FU.FIXTURE_CASES[name]
    scene, mesh = fixture_mesh(name, filtered, device)
    pts = mesh.vertices.cpu()[::stride].contiguous()
    assert pts.shape[0] > 500
    g, attr = M.scene_inputs(scene)
    got, ref = run_case(device, f"{name}{'_filtered' if filtered else ''}", g, attr, pts, nb, 2, level_set=not filtered)
    print(name, "density at the vertices: min", float(ref["density"].min()), "median", float(ref["density"].median()))
    return got


def check_extract_mesh(device, name="r32_nb8"):
    """extract_mesh(attributes=True): shapes, dtypes, ranges; bit for bit what mesh_attributes gives on the returned vertices; without
    the keyword the same mesh and no attributes."""
    n, r, nb, seed, _ = FU.FIXTURE_CASES[name]
    scene = FU.golden_scene(name)[1]
    pc = FU.make_model(scene, device)
    L = py_lib(device)
    plain = consumers.extract_mesh(pc, resolution=r, num_blocks=nb, lib=L, min_f=64, min_d=20, decimate_target=1500)
    assert plain.colors is None and plain.normals is None and plain.density is None
    mesh = pc.extract_mesh(resolution=r, num_blocks=nb, lib=L, min_f=64, min_d=20, decimate_target=1500, attributes=True)
    v = mesh.vertices.shape[0]
    assert torch.equal(mesh.vertices, plain.vertices) and torch.equal(mesh.faces, plain.faces) and v > 100
    for t, shape in ((mesh.colors, (v, 3)), (mesh.normals, (v, 3)), (mesh.density, (v,))):
        assert t.dtype == torch.float32 and tuple(t.shape) == shape and t.device == mesh.vertices.device and not t.requires_grad
    assert float(mesh.colors.min()) >= 0 and float(mesh.colors.max()) <= 1
    norm = torch.sqrt((mesh.normals.double() ** 2).sum(1))
    grad = M.raw(lib_of(device), device, *M.scene_inputs(scene), mesh.vertices.cpu(), nb, 2)[1]["grad"]
    nonzero = torch.from_numpy((np.abs(grad).sum(1) > 0))
    assert bool(nonzero.any()) and float((norm.cpu()[nonzero] - 1).abs().max()) <= 1e-6 and bool((norm.cpu()[~nonzero] == 0).all())
    again = pc.mesh_attributes(mesh.vertices, num_blocks=nb, lib=L)
    for k in ("colors", "normals", "density"):
        assert again[k].cpu().numpy().tobytes() == getattr(mesh, k).cpu().numpy().tobytes(), k
    with tempfile.TemporaryDirectory() as d:                                     # the coloured mesh goes to a file and comes back
        path = os.path.join(d, "m.ply")
        consumers.save_mesh_ply(path, mesh.vertices, mesh.faces, colors=mesh.colors, normals=mesh.normals)
        rv, rf, ra = consumers.load_mesh_ply(path, return_attributes=True)
        assert rv.tobytes() == mesh.vertices.cpu().numpy().tobytes() and rf.tobytes() == mesh.faces.cpu().numpy().tobytes()
        assert ra["normals"].tobytes() == mesh.normals.cpu().numpy().tobytes()
        assert (ra["colors"] == consumers.mesh_color_bytes(mesh.colors.cpu().numpy())).all()


# ---- order independence, determinism and outputs ----
def check_invariance(device):
    L = lib_of(device)
    g, attr = M.random_scene(500, 41)
    pts = M.random_points(300, 42)
    rc, base, _ = M.raw(L, device, g, attr, pts, 4, 1)
    assert rc == 0
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(43))
    rc, got, _ = M.raw(L, device, g, attr, pts[perm], 4, 1)
    assert rc == 0 and all(got[k].tobytes() == base[k][perm.numpy()].tobytes() for k in base)      # a permutation of the points
    sub = torch.arange(0, 300, 7)
    rc, got, _ = M.raw(L, device, g, attr, pts[sub], 4, 1)
    assert rc == 0 and all(got[k].tobytes() == base[k][sub.numpy()].tobytes() for k in base)       # a subset of the points
    # Gaussians appended outside every window: points in the -x half (cells 0, 1 of 4, reach 0), the additions in cell 3
    left = pts.clone()
    left[:, 0] = -left[:, 0].abs() - 0.01
    rc, base, _ = M.raw(L, device, g, attr, left, 4, 0)
    extra, eattr = M.random_scene(70, 44)
    extra["xyz"][:, 0] = extra["xyz"][:, 0].abs() * 0.4 + 0.6
    more = {k: (torch.cat((g[k], extra[k])) if torch.is_tensor(g[k]) else g[k]) for k in g}
    rc2, got, _ = M.raw(L, device, more, torch.cat((attr, eattr)), left, 4, 0)
    assert rc == 0 and rc2 == 0 and same(got, base)
    # each output alone
    rc, base, _ = M.raw(L, device, g, attr, pts, 4, 1)
    for k in ("density", "attr", "grad"):
        rc, got, _ = M.raw(L, device, g, attr, pts, 4, 1, want=(k,))
        assert rc == 0 and got[k].tobytes() == base[k].tobytes(), k
    # the Python call asks for what it is told to
    scene = FU.golden_scene("r32_nb8")[1]
    pc = FU.make_model(scene, device)
    p = M.random_points(100, 45, 0.7).to(device)
    full = mesh_attributes(pc, p, num_blocks=8, lib=py_lib(device))
    for k in ("colors", "normals", "density"):
        part = mesh_attributes(pc, p, num_blocks=8, want=(k,), lib=py_lib(device))
        assert list(part) == [k] and torch.equal(part[k], full[k])
    custom = mesh_attributes(pc, p, num_blocks=8, attr=torch.ones(scene["xyz"].shape[0], 3, device=device) * 0.5, want=("colors", "density"), lib=py_lib(device))
    live = custom["density"] > 0
    assert float((custom["colors"][live] - 0.5).abs().max()) <= 2 * (scene["xyz"].shape[0] + 1) * 2.0 ** -24 * 0.5     # the attr bar at n_p <= N


def check_arguments(device):
    """Every invalid-argument condition: -1 from the host-side check, the outputs untouched (nothing was launched)."""
    L = lib_of(device)
    g, attr = M.random_scene(50, 51)
    pts = M.random_points(20, 52)

    def spoil(field, value):
        def f(a):
            setattr(a, field, value)
        return f

    cases = [spoil(k, None) for k in ("xyz", "scaling", "rotation", "opacity", "attr", "points", "workspace")]
    cases += [spoil("N", 0), spoil("nb", 0), spoil("nb", 257), spoil("reach", -1), spoil("reach", 9), spoil("V", -1), spoil("V", 2 ** 30 + 1)]

    def small(a):
        a.workspace_bytes -= 1
    def misaligned(a):
        a.workspace = ctypes.c_void_p(a.workspace + 4)
    def no_output(a):
        a.density = a.attr_out = a.gradient = None
    for tweak in cases + [small, misaligned, no_output]:
        rc, _, whole = M.raw(L, device, g, attr, pts, 4, 1, tweak=tweak)
        assert rc == -1 and all((b == M.SENTINEL).all() for b in whole.values())
    assert L.dgs_mesh_attributes(None, None) == -1
    assert L.dgs_mesh_attributes_workspace_bytes(0, 4, 10) == 0 and L.dgs_mesh_attributes_workspace_bytes(5, 257, 10) == 0
    assert L.dgs_mesh_attributes_workspace_bytes(5, 4, 2 ** 30 + 1) == 0 and L.dgs_mesh_attributes_workspace_bytes(5, 4, 0) > 0
    pc = FU.make_model(FU.golden_scene("r32_nb8")[1], device)
    for bad in (dict(num_blocks=0), dict(num_blocks=300), dict(reach=9), dict(want=()), dict(want=("colour",))):
        with pytest.raises(ValueError):
            mesh_attributes(pc, pts.to(device), lib=py_lib(device), **bad)
    with pytest.raises(ValueError):
        mesh_attributes(pc, pts.double().to(device), lib=py_lib(device))


# SHA-256 of extract_fields(32, 8) and extract_mesh(resolution=32, num_blocks=8) on the filtered r32_nb8 fixture scene, minted on an MI355X
# with the library that has the parent commit's field.hip (tools/mesh_attr_error.py --parent-library, profiles/mesh_attr_parent_bytes.txt):
# what the gfx950 product library gave before the binning kernels moved into csrc/field_cells.h.  The emulated build is not pinned: its
# 2^x and the records' fp64 exp are the host's libm, whose results are not the same bits on every host.
PARENT_DIGESTS = {"occ": "97c2cc748a5862c092b21ba5b727025bdcd5ff85bb02e7797563c39b72e30bd7",
                  "vertices": "6b5be0dfe33263ad255f08e3ec93fb2a1a45a22a39a14a55e629f7b6e9c151b5",
                  "faces": "af5545cbeb2b0ce9ff4da41e36458111ab1b58ad71f1dd202439eddf76f3c51a"}


def check_defaults_unchanged(device):
    """extract_fields and extract_mesh() with default arguments: on the device the bytes the parent commit's library gave
    (PARENT_DIGESTS); everywhere the same bytes call after call and whether or not the attribute call ran in between on the same model
    (the binning kernels are shared with it)."""
    scene = FU.golden_scene("r32_nb8")[1]
    pc = FU.make_model(scene, device)
    L = py_lib(device)
    occ = consumers.extract_fields(pc, 32, 8, lib=L)
    mesh = consumers.extract_mesh(pc, resolution=32, num_blocks=8, lib=L)
    mesh_attributes(pc, mesh.vertices, num_blocks=8, lib=L)
    occ2 = consumers.extract_fields(pc, 32, 8, lib=L)
    mesh2 = consumers.extract_mesh(pc, resolution=32, num_blocks=8, lib=L)
    assert torch.equal(occ, occ2) and torch.equal(mesh.vertices, mesh2.vertices) and torch.equal(mesh.faces, mesh2.faces)
    assert mesh2.colors is None and consumers.Mesh(mesh.vertices, mesh.faces).normals is None
    if device != "cpu":
        import hashlib
        sha = lambda t: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
        got = {"occ": sha(occ), "vertices": sha(mesh.vertices), "faces": sha(mesh.faces)}
        assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and got == PARENT_DIGESTS, got
    ref64, counts = FU.field_ref64(scene, 32, 8)
    e32 = FU.e32_of(scene, 32, 8, ref64)
    FU.check_field("extract_fields after the header move", FU.gather_blocks(occ, 8, FU.all_blocks(8)), ref64, counts, e32)


# ---- the emulated runs ----
def test_trivial_sizes_emulated():
    check_trivial("cpu")


def test_sphere_emulated():
    check_sphere("cpu")


def test_three_blobs_emulated():
    check_blobs("cpu")


def test_crowded_cells_emulated():
    check_crowded("cpu")


def test_window_edges_emulated():
    check_edges("cpu")


@pytest.mark.parametrize("name,filtered", [("r32_nb8", False), ("r32_nb8", True), ("r40_nb4", False), ("r40_nb4", True)])
def test_fixture_scene_emulated(name, filtered):
    check_fixture("cpu", name, filtered)


def test_extract_mesh_with_attributes_emulated():
    check_extract_mesh("cpu")


def test_invariance_emulated():
    check_invariance("cpu")


def test_argument_checks_emulated():
    check_arguments("cpu")


def test_defaults_unchanged_emulated():
    check_defaults_unchanged("cpu")


# ---- PLY ----
HAND_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
HAND_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)


def test_ply_without_attributes_is_the_old_file():
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              "element face 4\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    faces = b"".join(b"\x03" + row.astype("<i4").tobytes() for row in HAND_F)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "m.ply")
        consumers.save_mesh_ply(path, HAND_V, HAND_F)
        assert open(path, "rb").read() == header + HAND_V.astype("<f4").tobytes() + faces
        v, f = consumers.load_mesh_ply(path)
        assert v.tobytes() == HAND_V.tobytes() and f.tobytes() == HAND_F.tobytes()
        assert consumers.load_mesh_ply(path, return_attributes=True)[2] == {}


@pytest.mark.parametrize("with_colors,with_normals", [(True, False), (False, True), (True, True)])
def test_ply_round_trip(with_colors, with_normals):
    colors = np.array([[0.0, 0.5, 1.0], [0.25, 1.2, -0.1], [0.999, 0.001, 0.5], [1 / 3, 2 / 3, 0.1]], dtype=np.float32)
    normals = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0.0, -0.8]], dtype=np.float32)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sub", "m.ply")
        consumers.save_mesh_ply(path, torch.from_numpy(HAND_V), torch.from_numpy(HAND_F), colors=torch.from_numpy(colors) if with_colors else None,
                                normals=normals if with_normals else None)
        v, f = consumers.load_mesh_ply(path)
        v2, f2, at = consumers.load_mesh_ply(path, return_attributes=True)
        assert v.tobytes() == HAND_V.tobytes() == v2.tobytes() and f.tobytes() == HAND_F.tobytes() == f2.tobytes()
        assert sorted(at) == ["colors"] * with_colors + ["normals"] * with_normals
        if with_colors:
            assert at["colors"].dtype == np.uint8 and (at["colors"] == consumers.mesh_color_bytes(colors)).all()
        if with_normals:
            assert at["normals"].dtype == np.float32 and at["normals"].tobytes() == normals.tobytes()
        size = 12 + 12 * with_normals + 3 * with_colors
        assert os.path.getsize(path) == open(path, "rb").read().index(b"end_header\n") + 11 + 4 * size + 4 * 13


def test_ply_colour_rounding():
    eps = 1e-9
    c = np.array([0.0, 0.5 / 255, 1 / 255 - eps, 1.0, 1.2, -0.1], dtype=np.float64)
    assert consumers.mesh_color_bytes(c).tolist() == [0, 1, 1, 255, 255, 0]
    assert consumers.mesh_color_bytes(np.array([0.5 / 255 - eps, 254.5 / 255 - eps, 0.5])).tolist() == [0, 254, 128]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                         # no undefined cast of a non-finite value
        assert consumers.mesh_color_bytes(np.array([np.nan, np.inf, -np.inf, 0.25], dtype=np.float32)).tolist() == [0, 255, 0, 64]


# ---- ABI ----
def test_abi():
    from emu_util import emu_lib
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "dgs_mesh_attr.h")).read()
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(_native.MESH_ATTR_SYMBOLS) and len(names) == 2
    for lib in (emu_lib(), _native.lib()):
        for name in names:
            assert hasattr(lib, name), name
    src = '#include <stdio.h>\n#include "dgs_mesh_attr.h"\nint main(){printf("%zu\\n", sizeof(DgsMeshAttrArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + inc, c, "-o", exe])
        assert ctypes.sizeof(_native.DgsMeshAttrArgs) == int(subprocess.check_output([exe]))
