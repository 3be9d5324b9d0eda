"""Mesh smoothing by Taubin's lambda | mu passes (csrc/mesh_smooth.hip, include/dgs_mesh_smooth.h, dgs_amd.consumers.smooth_mesh,
extract_mesh(smooth_iterations)) on the CPU-emulated build of the kernels: every output byte and all four counts against the numpy
restatement of tests/mesh_smooth_util.py.  The checks are functions of a device, which tests/test_mesh_smooth_gpu.py runs on the GPU.

Sizes.  Every kernel of csrc/mesh_smooth.hip runs workgroups of 256 threads, one row a thread; a wave is 64 rows, a scan block 256
rows, and the scan over the block totals gives each of its 1,024 threads one block up to 1,024 blocks.  So the strips have 63, 64, 65
vertices (a wave), 255, 256, 257 (a workgroup and a scan block) and 65,537 (257 scan blocks); noise64_05 on the device has 1,567
blocks of vertices, more than the 1,024 threads of that scan.  A vertex of up to 48 faces takes a thread and one of more a wave, and
one of more than 16,384 does not move: the fans have 47, 48, 49 and 16,384, 16,385 faces."""
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
import mesh_smooth_util as S  # noqa: E402
from dgs_amd import _native, consumers  # noqa: E402
from dgs_amd.consumers import smooth_mesh  # noqa: E402  (without the feature the module fails here)

assert _native.MESH_SMOOTH_SYMBOLS


def lib_of(device):
    if device == "cpu":
        from emu_util import emu_lib
        return emu_lib()
    return _native.lib()


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check(device, vertices, faces, **kw):
    """The raw call against the restatement, exactly; a second call gives the same bytes; the Python call gives the same tensor and
    the same counts.  -> the restatement's result."""
    L = lib_of(device)
    want = S.restatement(vertices, faces, **kw)
    got = S.smooth_raw(L, vertices, faces, device, **kw)
    print("V", np.shape(vertices)[0], "F", np.shape(faces)[0], kw if "fixed" not in kw else "fixed", "counts", got["counts"], "restated", want["counts"])
    S.assert_identical(got, want)
    S.assert_identical(S.smooth_raw(L, vertices, faces, device, **kw), got)
    tv = torch.from_numpy(np.array(vertices, dtype=np.float32).reshape(-1, 3)).to(device)
    tf = torch.from_numpy(np.array(faces, dtype=np.int32).reshape(-1, 3)).to(device)
    pk = dict(kw)
    if "fixed" in pk:
        pk["fixed"] = torch.from_numpy(np.array(pk["fixed"], dtype=np.uint8)).to(device)
    out, counts = smooth_mesh(tv, tf, return_counts=True, lib=None if device != "cpu" else L, **pk)
    assert out.dtype == torch.float32 and out.device == tv.device and tuple(out.shape) == tuple(tv.shape) and not out.requires_grad
    S.assert_identical(dict(vertices=out.cpu().numpy(), counts=counts), want)
    return want


# ---- the cases: name -> (vertices, faces, keyword arguments) ----
def _grid(nx, ny):
    x, y = np.meshgrid(np.arange(nx + 1) * 1.0, np.arange(ny + 1) * 1.0, indexing="ij")
    v = np.stack((x.ravel(), y.ravel(), np.sin(x.ravel() * 1.7) * np.cos(y.ravel() * 2.3)), axis=1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).ravel()
    b, c, d = a + (ny + 1), a + (ny + 2), a + 1
    return v, np.concatenate((np.stack((a, b, c), axis=1), np.stack((a, c, d), axis=1))).astype(np.int32)


FAR = 1.0e6
MIXED_BAD, MIXED_NULL, MIXED_UNREFERENCED = 6, 4, 3


def _mixed():
    """A bumpy sheet with unreferenced vertices in front, inside and behind, invalid faces (an index of -1, of V, of 2^31 - 1), null
    faces and duplicated faces in between."""
    gv, gf = _grid(6, 6)
    pad = np.array([[FAR, -FAR, FAR]], dtype=np.float32)
    v = np.concatenate((pad, gv[:20], -pad, gv[20:], pad))
    gf = np.where(gf < 20, gf + 1, gf + 2).astype(np.int32)
    V = v.shape[0]
    bad = np.array([[-1, 1, 2], [2, V, 3], [4, 5, 2 ** 31 - 1], [-2 ** 31, -1, V], [V, V, V], [0, V, 0]], dtype=np.int32)
    null = np.array([[3, 3, 5], [2, 7, 2], [4, 4, 4], [9, 8, 8]], dtype=np.int32)
    return v, np.concatenate((gf[:7], bad[:2], null[:1], gf[7:30], gf[:5], bad[2:5], null[1:3], gf[30:], gf[3:5], bad[5:], null[3:])).astype(np.int32)


def _clustered(name, n):
    out = D.restatement(*S.level_set(name), n)
    return out["vertices"], out["faces"]


def _half_fixed(name):
    v, f = S.level_set(name)
    return v, f, dict(fixed=(np.arange(v.shape[0]) % 2).astype(np.uint8))


CLUSTERED_INCIDENCE = {"sphere_clustered_8": 10, "noise24_05_clustered_11": 30}
CASES = {
    "strip61": lambda: S.strip(61) + ({},),
    "strip62": lambda: S.strip(62) + ({},),
    "strip63": lambda: S.strip(63) + ({},),
    "strip253": lambda: S.strip(253) + ({},),
    "strip254": lambda: S.strip(254) + ({},),
    "strip255": lambda: S.strip(255) + ({},),
    "strip65535": lambda: S.strip(65535) + (dict(iterations=2),),
    "fans_47_48_49": lambda: S.fans([S.THREAD_MAX - 1, S.THREAD_MAX, S.THREAD_MAX + 1]) + ({},),
    "fans_16384_16385": lambda: S.fans([S.CAP, S.CAP + 1]) + (dict(iterations=2),),
    "mixed": lambda: _mixed() + ({},),
    "sphere": lambda: S.level_set("sphere") + ({},),
    "torus": lambda: S.level_set("torus") + ({},),
    "blobs": lambda: S.level_set("blobs") + ({},),
    "noise24_05": lambda: S.level_set("noise24_05") + ({},),
    "sphere_clustered_8": lambda: _clustered("sphere", 8) + ({},),
    "noise24_05_clustered_11": lambda: _clustered("noise24_05", 11) + ({},),
    "blobs_half_fixed": lambda: _half_fixed("blobs"),
    "torus_iterations_0": lambda: S.level_set("torus") + (dict(iterations=0),),
    "torus_iterations_1": lambda: S.level_set("torus") + (dict(iterations=1),),
    "torus_laplacian": lambda: S.level_set("torus") + (dict(mu=0.0),),
    "torus_both_zero": lambda: S.level_set("torus") + (dict(lam=0.0, mu=0.0),),
    "torus_lambda_zero": lambda: S.level_set("torus") + (dict(lam=0.0, iterations=3),),
}


def check_case(device, name):
    v, f, kw = CASES[name]()
    want = check(device, v, f, **kw)
    V, F = v.shape[0], f.shape[0]
    out, counts = want["vertices"], want["counts"]
    c = S.incidence(V, f)["c"]
    if name.startswith("strip"):
        assert F == int(name[5:]) and V == F + 2 and counts == [0, 0, 0, 0] and int(c.max()) == 3
        assert not same_bytes(out, v)
    if name == "fans_47_48_49":                                               # the hubs: one below, one at, one above the thread / wave threshold
        hubs = [0, S.THREAD_MAX + 1, 2 * S.THREAD_MAX + 3]
        assert [int(c[h]) for h in hubs] == [S.THREAD_MAX - 1, S.THREAD_MAX, S.THREAD_MAX + 1] and counts == [0, 0, 0, 0]
        assert all(not same_bytes(out[h], v[h]) for h in hubs)
    if name == "fans_16384_16385":                                            # the second hub is above the cap: its input bytes, counted
        first, second = 0, S.CAP + 2
        assert int(c[first]) == S.CAP and int(c[second]) == S.CAP + 1 and counts == [0, 0, 1, 0]
        assert same_bytes(out[second], v[second]) and not same_bytes(out[first], v[first])
        assert not same_bytes(out[second + 1:], v[second + 1:])               # its ring moves, with the hub as a neighbour
    if name == "mixed":
        assert counts == [MIXED_BAD, MIXED_NULL, 0, MIXED_UNREFERENCED]
        far = np.abs(v).max(axis=1) == FAR
        assert int(far.sum()) == MIXED_UNREFERENCED and same_bytes(out[far], v[far]) and float(np.abs(out[~far]).max()) <= 7.0
        assert int(c.max()) > 6                                               # the duplicated faces count as often as they occur
        gv, gf = _grid(6, 6)
        f6 = np.concatenate((gf, gf[:5], gf[3:5]))
        alone = S.restatement(gv, f6)                                         # as without the invalid and null faces and the far vertices
        assert same_bytes(out[~far], alone["vertices"])
    if name in CLUSTERED_INCIDENCE:
        assert int(c.max()) == CLUSTERED_INCIDENCE[name] and counts == [0, 0, 0, 0]
    if name == "blobs_half_fixed":
        odd = np.arange(V) % 2 == 1
        assert same_bytes(out[odd], v[odd]) and not same_bytes(out[~odd], v[~odd])
    if name in ("torus_iterations_0", "torus_both_zero"):                     # the input bytes
        assert same_bytes(out, v)
    if name in ("torus_iterations_1", "torus_laplacian", "torus_lambda_zero", "sphere", "blobs", "noise24_05"):
        assert not same_bytes(out, v) and counts == [0, 0, 0, 0]


EMULATED = [n for n in CASES]


@pytest.mark.parametrize("name", EMULATED)
def test_case_emulated(name):
    check_case("cpu", name)


def check_empty(device):
    L = lib_of(device)
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    some_v, some_f = S.strip(2)
    for v, f, counts in ((none_v, none_f, [0, 0, 0, 0]), (some_v, none_f, [0, 0, 0, 4]), (none_v, some_f, [2, 0, 0, 0])):
        got = S.smooth_raw(L, v, f, device)
        assert got["counts"] == counts and same_bytes(got["vertices"], v)
        S.assert_identical(got, S.restatement(v, f))
        out, c = smooth_mesh(torch.from_numpy(v.copy()).to(device), torch.from_numpy(f.copy()).to(device), return_counts=True, lib=None if device != "cpu" else L)
        assert tuple(out.shape) == v.shape and out.dtype == torch.float32 and c == counts and same_bytes(out.cpu().numpy(), v)


def test_empty_meshes_emulated():
    check_empty("cpu")


def check_invariance(device):
    """On blobs: renaming the vertices permutes the output rows and changes no byte; permuting the faces, rotating or reversing their
    corners changes nothing."""
    L = lib_of(device)
    v, f = S.level_set("blobs")
    base = S.smooth_raw(L, v, f, device)
    rng = np.random.default_rng(5)
    perm = rng.permutation(v.shape[0])                                        # vertex i becomes perm[i]
    moved = np.empty_like(v)
    moved[perm] = v
    got = S.smooth_raw(L, moved, perm[f].astype(np.int32), device)
    assert got["counts"] == base["counts"] and same_bytes(got["vertices"][perm], base["vertices"])
    turn = rng.integers(0, 3, size=f.shape[0])
    rotated = np.stack([f[np.arange(f.shape[0]), (turn + k) % 3] for k in range(3)], axis=1)
    for other in (f[rng.permutation(f.shape[0])], rotated, f[:, ::-1], rotated[rng.permutation(f.shape[0])][:, ::-1]):
        S.assert_identical(S.smooth_raw(L, v, np.ascontiguousarray(other), device), base)
    S.assert_identical(base, S.restatement(v, f))


def test_invariance_emulated():
    check_invariance("cpu")


def assert_smooths(smooth):
    """The properties that do not trust the restatement, on the voxel ball (1,258 vertices, 2,512 faces) at the defaults; smooth(v, f,
    **kw) -> vertices.  Conditions with margin (measured with the restatement: spread 0.2029 -> 0.1124, mean radius 8.2019 -> 8.2134,
    Laplacian 7.9422), not tolerances on the kernel: the kernel is compared bit for bit."""
    v, f, centre = S.voxel_ball()
    assert v.shape[0] == 1258 and f.shape[0] == 2512
    mean0, std0 = S.radius_stats(v, centre)
    mean1, std1 = S.radius_stats(smooth(v, f), centre)
    mean2, _ = S.radius_stats(smooth(v, f, mu=0.0), centre)
    print("radius mean, spread: input", mean0, std0, "Taubin", mean1, std1, "Laplacian mean", mean2)
    assert std1 <= 0.65 * std0                                                # the staircases go
    assert abs(mean1 - mean0) <= 0.005 * mean0                                # Taubin keeps the size
    assert mean2 < 0.98 * mean0                                               # plain Laplacian smoothing shrinks


def test_restatement_smooths_without_shrinking():
    assert_smooths(lambda v, f, **kw: S.restatement(v, f, **kw)["vertices"])


def check_smooths(device):
    L = lib_of(device)
    assert_smooths(lambda v, f, **kw: S.smooth_raw(L, v, f, device, **kw)["vertices"])


def test_smooths_without_shrinking_emulated():
    check_smooths("cpu")


class Watched:
    """The library with every call of a dgs_mesh_smooth* symbol written down."""

    def __init__(self, L):
        self._L, self.calls = L, []

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("dgs_mesh_smooth"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def check_extract_mesh(device, case, target):
    """extract_mesh(smooth_iterations=3) moves the vertices of the unsmoothed call's mesh as smooth_mesh does and keeps its faces; the
    attributes are evaluated at the smoothed vertices; the default path calls none of the new symbols and returns the same bytes."""
    L = Watched(lib_of(device))
    n, r, nb, seed, sampled = FU.FIXTURE_CASES[case]
    scene, _ = FU.golden_scene(case)
    pc = FU.make_model(scene, device).apply_all_filters(**FU.PIPELINE_FILTERS)
    kw = dict(min_f=8, min_d=0, decimate_target=target)
    plain = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, **kw)
    zero = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, smooth_iterations=0, **kw)
    assert L.calls == []                                                      # the paths of before launch what they launched
    assert torch.equal(zero.vertices, plain.vertices) and torch.equal(zero.faces, plain.faces) and 0 < plain.faces.shape[0] <= target
    mesh = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, smooth_iterations=3, smooth_lambda=0.4, smooth_mu=-0.45, **kw)
    assert L.calls == ["dgs_mesh_smooth_workspace_bytes", "dgs_mesh_smooth"]
    want = smooth_mesh(plain.vertices, plain.faces, 3, 0.4, -0.45, lib=L)
    assert torch.equal(mesh.vertices, want) and torch.equal(mesh.faces, plain.faces) and not torch.equal(mesh.vertices, plain.vertices)
    assert mesh.colors is None and mesh.vertices.device == plain.vertices.device
    S.assert_identical(dict(vertices=want.cpu().numpy(), counts=None),
                       dict(S.restatement(plain.vertices.cpu().numpy(), plain.faces.cpu().numpy(), 3, 0.4, -0.45), counts=None))
    default = consumers.extract_mesh(pc, FU.LEVEL, r, nb, lib=L, smooth_iterations=3)                # the defaults of the weights
    assert torch.equal(default.vertices, smooth_mesh(pc.extract_mesh(FU.LEVEL, r, nb, lib=L).vertices, default.faces, 3, lib=L))
    full = pc.extract_mesh(FU.LEVEL, r, nb, lib=L, smooth_iterations=3, smooth_lambda=0.4, smooth_mu=-0.45, attributes=True, **kw)
    assert torch.equal(full.vertices, want) and torch.equal(full.faces, plain.faces)
    at = pc.mesh_attributes(want, num_blocks=nb, lib=L)
    for k in ("colors", "normals", "density"):
        assert at[k].cpu().numpy().tobytes() == getattr(full, k).cpu().numpy().tobytes(), k
    print(case, "faces", tuple(plain.faces.shape), "largest move", float((want - plain.vertices).abs().max()))


def test_extract_mesh_with_the_smoothing_emulated():
    check_extract_mesh("cpu", "r32_nb8", 1500)


def test_invalid_arguments():
    """Each DGS_ERR_INVALID_ARGUMENT case returns that status and writes nothing: counts, output and workspace keep their fill."""
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x.copy()) for x in S.strip(6))
    need = L.dgs_mesh_smooth_workspace_bytes(v.shape[0], f.shape[0])
    assert need > 0 and need % 16 == 0
    for V, F in ((-1, 5), (5, -1), ((1 << 30) + 1, 5), (5, (1 << 29) + 1)):
        assert L.dgs_mesh_smooth_workspace_bytes(V, F) == 0, (V, F)
    assert L.dgs_mesh_smooth_workspace_bytes(1 << 30, 1 << 29) > 0 and L.dgs_mesh_smooth_workspace_bytes(0, 0) > 0
    ws, ws_ptr = S._guarded(need, "cpu")
    cnt, cnt_ptr = S._guarded(16, "cpu")
    ov, ov_ptr = S._guarded(12 * 8, "cpu")

    def args(**over):
        a = S.make_args(L, v, f, 2, 0.5, -0.53, None, ws_ptr, need, cnt_ptr, ov_ptr)
        for k, x in over.items():
            setattr(a, k, x)
        return ctypes.byref(a)

    bad = (dict(V=-1), dict(F=-1), dict(V=(1 << 30) + 1), dict(F=(1 << 29) + 1), dict(iterations=-1), dict(iterations=(1 << 20) + 1),
           dict(lam=float("nan")), dict(mu=float("inf")), dict(vertices=None), dict(faces=None), dict(out_vertices=None), dict(workspace=None),
           dict(workspace_bytes=need - 16), dict(workspace=ws_ptr + 8), dict(V=9), dict(F=7),             # more rows need more workspace
           dict(out_vertices=v.data_ptr()), dict(out_vertices=v.data_ptr() + 12 * 7), dict(out_vertices=v.data_ptr() - 12 * 7))
    for over in bad:
        assert L.dgs_mesh_smooth(args(**over), None) == -1, over              # DGS_ERR_INVALID_ARGUMENT
    assert L.dgs_mesh_smooth(None, None) == -1
    assert all(S._guards_intact(t, 0) for t in (ws, cnt, ov))
    before = v.numpy().copy()
    assert L.dgs_mesh_smooth(args(), None) == 0 and L.dgs_mesh_smooth(args(counts=None), None) == 0   # the counts are optional
    assert cnt.numpy()[S.BAND:S.BAND + 16].copy().view(np.uint32).tolist() == [0, 0, 0, 0]
    assert S._guards_intact(ws, need) and S._guards_intact(cnt, 16) and S._guards_intact(ov, 96) and np.array_equal(v.numpy(), before)
    got = ov.numpy()[S.BAND:S.BAND + 96].copy().view(np.float32).reshape(8, 3)
    assert same_bytes(got, S.restatement(before, f.numpy(), 2)["vertices"])


def test_python_checks():
    from emu_util import emu_lib
    L = emu_lib()
    v, f = (torch.from_numpy(x.copy()) for x in S.level_set("torus"))
    for bad_v, bad_f in ((v.double(), f), (v, f.long()), (v[:, :2], f), (v, f[:, :2]), (v.reshape(-1), f), (v, f.reshape(-1))):
        with pytest.raises(ValueError):
            smooth_mesh(bad_v, bad_f, lib=L)
    with pytest.raises(RuntimeError, match="rebuild"):                       # a library from before the feature
        smooth_mesh(v, f, lib=types.SimpleNamespace())
    for kw in (dict(iterations=-1), dict(iterations=2.5), dict(iterations=(1 << 20) + 1), dict(lam=float("nan")), dict(mu=float("inf")),
               dict(fixed=torch.zeros(v.shape[0] - 1, dtype=torch.uint8)), dict(fixed=torch.zeros(v.shape[0], dtype=torch.int32)),
               dict(fixed=torch.zeros((v.shape[0], 1), dtype=torch.bool))):
        with pytest.raises(ValueError):
            smooth_mesh(v, f, lib=L, **kw)
    out = smooth_mesh(v.clone().requires_grad_(True), f, 2, lib=L)
    assert tuple(out.shape) == tuple(v.shape) and not out.requires_grad and out is not v
    mask = torch.arange(v.shape[0]) % 3 == 0                                  # a bool mask is the uint8 mask
    assert torch.equal(smooth_mesh(v, f, 2, fixed=mask, lib=L), smooth_mesh(v, f, 2, fixed=mask.to(torch.uint8), lib=L))
    assert torch.equal(smooth_mesh(v, f, 2, fixed=mask, lib=L)[mask], v[mask])
    out, counts = smooth_mesh(v, f, 0, return_counts=True, lib=L)
    assert torch.equal(out, v) and counts == [0, 0, 0, 0]
    strided = torch.zeros((v.shape[0], 6))[:, ::2]                            # not contiguous: taken as it reads
    strided.copy_(v)
    assert torch.equal(smooth_mesh(strided, f, 2, lib=L), smooth_mesh(v, f, 2, lib=L))


def test_abi():
    from emu_util import emu_lib
    inc = os.path.join(ROOT, "include")
    text = open(os.path.join(inc, "dgs_mesh_smooth.h")).read()
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert names == sorted(_native.MESH_SMOOTH_SYMBOLS) and len(names) == 2
    for lib in (emu_lib(), _native.lib()):
        for name in names:
            assert hasattr(lib, name), name
    flowed = re.sub(r"\s*\n \*\s*", " ", text)                               # the comment as running text
    for phrase in ("Renaming the vertices", "Permuting the faces changes nothing", "Rotating or reversing the corners of a face changes nothing",
                   "VCG moves them along the border only", "no border handling, no cotangent weights, no remeshing"):
        assert phrase in flowed, phrase
    src = '#include <stdio.h>\n#include "dgs_mesh_smooth.h"\nint main(){printf("%zu\\n", sizeof(DgsMeshSmoothArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + inc, c, "-o", exe])
        assert ctypes.sizeof(_native.DgsMeshSmoothArgs) == int(subprocess.check_output([exe]))
