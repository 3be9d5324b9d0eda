"""Gaussian density field and the GaussianModel filters (csrc/field.hip, dgs_amd.consumers.extract_fields, dgs_amd.denoiser.GaussianModel)
on the CPU-emulated build of the kernels, against tests/golden/field_ref.npz (the reference's own masks and fp32 field,
tools/make_field_golden.py) and the fp64 restatement in tests/field_util.py (bounds: there)."""
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

import field_util as U  # noqa: E402


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    """-> (filtered scene, blocks, ref64, counts, e32, reference's fp32 blocks): computed once per case, shared, never modified."""
    n, r, nb, seed, sampled = U.FIXTURE_CASES[name]
    _, kept = U.golden_scene(name)
    blocks = U.golden_blocks(name)
    ref64, counts = U.field_ref64(kept, r, nb, blocks=blocks)
    ref32 = torch.from_numpy(U.golden()[f"{name}/occ"])
    if sampled is None:
        ref32 = U.gather_blocks(ref32, nb, blocks)
    e32 = float((ref32.double() - ref64).abs().max())
    return kept, blocks, ref64, counts, e32, ref32


def check_fixture_case(name, lib, device, report=None, twice=True):
    """apply_all_filters with the pipeline's arguments, then extract_fields, on `device`: surviving set, mesh_center / mesh_scale and
    the field against the fixture and the restatement; a second call gives the same bits."""
    n, r, nb, seed, sampled = U.FIXTURE_CASES[name]
    g = U.golden()
    scene, _ = U.golden_scene(name)
    kept, blocks, ref64, counts, e32, _ = fixture_reference(name)
    pc = U.make_model(scene, device)
    assert pc.apply_all_filters(**U.PIPELINE_FILTERS) is pc
    assert pc._xyz.shape[0] == int(g[f"{name}/counts"][1])
    for k, t in (("xyz", pc._xyz), ("scaling", pc._scaling), ("rotation", pc._rotation), ("opacity", pc._opacity)):
        assert torch.equal(t.cpu(), kept[k]), k
    occ = pc.extract_fields(r, nb, lib=lib)
    assert occ.shape == (r, r, r) and occ.dtype == torch.float32 and occ.device == pc._xyz.device
    assert torch.equal(pc.mesh_center.cpu(), torch.from_numpy(g[f"{name}/mesh_center"])) and pc.mesh_scale == float(g[f"{name}/mesh_scale"])
    out = U.check_field(name, U.gather_blocks(occ, nb, blocks), ref64, counts, e32, report)
    if twice:
        assert torch.equal(pc.extract_fields(r, nb, lib=lib), occ)
    return out


def check_sampled_case(name, scene, r, nb, blocks, lib, device, report=None, min_nonempty=0):
    """A scene without a fixture: e32 from the fp32 evaluation of the restatement; two calls bit-identical; finite."""
    ref64, counts = U.field_ref64(scene, r, nb, blocks=blocks)
    assert int((counts > 0).sum()) >= min_nonempty, (int((counts > 0).sum()), min_nonempty)
    e32 = U.e32_of(scene, r, nb, ref64, blocks=blocks)
    pc = U.make_model(scene, device)
    occ = pc.extract_fields(r, nb, lib=lib)
    assert bool(torch.isfinite(occ).all())
    out = U.check_field(name, U.gather_blocks(occ, nb, blocks), ref64, counts, e32, report)
    assert torch.equal(pc.extract_fields(r, nb, lib=lib), occ)
    return out, occ, counts, ref64


@pytest.mark.parametrize("name", list(U.FIXTURE_CASES))
def test_restatement_is_pinned_to_the_reference(name):
    """The reference's fp32 field sits within fp32 evaluation error of the fp64 restatement: per term a few roundings of the quadratic
    form and the exponential (8 * 2^-24 of the term), pairwise summation of n_b terms (log2 n_b * 2^-24 of the sum)."""
    _, _, ref64, counts, e32, ref32 = fixture_reference(name)
    top = float(ref64.max())
    print(f"{name}: e32 {e32:.3e} = {e32 / top:.3e} of the field's max {top:.4g}")
    assert e32 <= (8 + math.log2(int(counts.max()))) * 2.0 ** -24 * top
    assert int(((ref32 > U.LEVEL) != (ref64 > U.LEVEL)).sum()) == 0
    assert bool((ref32[counts == 0] == 0).all())


@pytest.mark.parametrize("name", list(U.FIXTURE_CASES))
def test_filters_match_the_reference_masks(name):
    g = U.golden()
    scene, kept = U.golden_scene(name)
    pc = U.make_model(scene)
    before = pc._xyz
    assert pc.prune(0.02) is pc and pc._xyz is not before                     # in place, returns self
    prune = torch.from_numpy(g[f"{name}/mask_prune"])
    assert pc._xyz.shape[0] == int(g[f"{name}/counts"][0]) == int(prune.sum())
    for k, t in (("xyz", pc._xyz), ("scaling", pc._scaling), ("rotation", pc._rotation), ("opacity", pc._opacity), ("features", pc._features_dc)):
        assert torch.equal(t.reshape(t.shape[0], -1), scene[k][prune].reshape(t.shape[0], -1)), k
    assert pc.crop(U.PIPELINE_FILTERS["crop_bbx"]) is pc
    assert torch.equal(pc._xyz, scene["xyz"][prune][torch.from_numpy(g[f"{name}/mask_crop"])])
    chained = U.make_model(scene).prune(0.02).crop(U.PIPELINE_FILTERS["crop_bbx"])
    both = U.make_model(scene).apply_all_filters(**U.PIPELINE_FILTERS)
    for k in ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity"):
        assert torch.equal(getattr(chained, k), getattr(pc, k)) and torch.equal(getattr(both, k), getattr(pc, k)), k
    assert torch.equal(pc._xyz, kept["xyz"]) and pc._features_rest is None
    m = torch.zeros(pc._xyz.shape[0], dtype=torch.bool)
    m[::3] = True
    assert pc.filter(m) is pc and torch.equal(pc._opacity, kept["opacity"][m])
    assert U.make_model(scene).to("cpu")._xyz.device.type == "cpu"


def test_nearfar_shrink_and_covariance_match_their_torch_expressions():
    scene = U.make_scene(1500, 7)
    cams = torch.tensor([[2.7, 0.0, 0.0], [0.0, 2.7, 0.0], [-1.9, -1.9, 0.3]])
    pc = U.make_model(scene)
    assert pc.prune_by_nearfar(cams, (0.01, 0.99)) is pc
    d = torch.cdist(scene["xyz"][None], cams[None])[0]
    q = torch.quantile(d, torch.tensor((0.01, 0.99)), dim=0)
    keep = ~((d < q[0:1]) | (d > q[1:2])).any(dim=1)
    assert 0 < int(keep.sum()) < 1500 and torch.equal(pc._xyz, scene["xyz"][keep]) and torch.equal(pc._rotation, scene["rotation"][keep])
    # apply_all_filters runs the near/far step last, on what prune and crop left, with its own default percentiles
    pc = U.make_model(scene).apply_all_filters(0.02, [-1, 1, -1, 1, -1, 1], cam_origins=cams)
    two = U.make_model(scene).prune(0.02).crop().prune_by_nearfar(cams, (0.005, 1.0))
    assert torch.equal(pc._xyz, two._xyz) and pc._xyz.shape[0] < U.make_model(scene).prune(0.02).crop()._xyz.shape[0]
    pc = U.make_model(scene)
    assert pc.shrink_bbx(0.05) is pc
    lo, hi = torch.quantile(scene["xyz"], torch.tensor([0.05, 0.95]).float(), dim=0)
    keep = ((scene["xyz"] >= lo) & (scene["xyz"] <= hi)).all(dim=1)
    assert torch.equal(pc._xyz, scene["xyz"][keep]) and 0 < pc._xyz.shape[0] < 1500
    # get_covariance: (R S)(R S)^T of the reference's build_scaling_rotation, [N, 6]
    pc = U.make_model(scene, scaling_modifier=0.5)
    cov = pc.get_covariance(2)
    ref = torch.stack(U._cov6(2 * (torch.exp(scene["scaling"].double()) * 0.5), scene["rotation"].double()), dim=1)
    assert cov.shape == (1500, 6) and float((cov.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


@pytest.mark.parametrize("name", list(U.FIXTURE_CASES))
def test_field_matches_the_reference_emulated(name):
    from emu_util import emu_lib
    check_fixture_case(name, emu_lib(), "cpu", twice=name != "r64_nb16")      # the large case takes the emulator 3 s a call


def test_blocks_without_members_are_exactly_zero():
    """Narrow member boxes (nb = 16 at R = 32: split 2, lanes idle) leave most of the grid without members."""
    from emu_util import emu_lib
    scene = U.make_scene(400, 11)
    scene = {k: v[50:] for k, v in scene.items()}                                # the shell only
    _, occ, counts, ref64 = check_sampled_case("r32_nb16", scene, 32, 16, U.all_blocks(16), emu_lib(), "cpu")
    zero_blocks = U.gather_blocks(occ, 16, U.all_blocks(16)).reshape(16 ** 3, -1).abs().max(dim=1).values == 0
    assert 0 < int((counts == 0).sum()) < 16 ** 3
    # the zero blocks are the member-less ones, and those whose few small members are all more than ~13 sigma from every voxel
    # (each term below fp32's normal range: check_field holds every zero voxel to that)
    assert bool(zero_blocks[counts == 0].all())
    assert not bool(zero_blocks[ref64.reshape(16 ** 3, -1).max(dim=1).values > 2.0 ** -100].any())


def test_split_one_and_odd_split():
    from emu_util import emu_lib
    scene = {k: v[30:] for k, v in U.make_scene(300, 12).items()}
    check_sampled_case("r8_nb8", scene, 8, 8, U.all_blocks(8), emu_lib(), "cpu")             # split 1
    check_sampled_case("r24_nb8", scene, 24, 8, U.all_blocks(8), emu_lib(), "cpu")           # split 3: 27 of a wave's 64 lanes, 2 waves of 4 blocks
    check_sampled_case("r22_nb2", scene, 22, 2, U.all_blocks(2), emu_lib(), "cpu")           # split 11: two passes of 1024 voxels


def _probe_scene(x):
    """Two anchors at -+0.9 on every axis (mesh_center 0, mesh_scale exactly 1 in fp32: normalised = raw) and one wide Gaussian at
    (x, 0.1, 0.1)."""
    xyz = torch.tensor([[-0.9, -0.9, -0.9], [0.9, 0.9, 0.9], [x, 0.1, 0.1]], dtype=torch.float32)
    scaling = torch.log(torch.tensor([[0.02] * 3, [0.02] * 3, [0.5] * 3]))
    rotation = torch.tensor([[1.0, 0, 0, 0]] * 3)
    opacity = torch.tensor([[1.0], [1.0], [2.0]])
    return dict(xyz=xyz, features=torch.zeros(3, 1, 3), scaling=scaling, rotation=rotation, opacity=opacity)


def test_membership_is_a_strict_comparison_with_the_block_bounds():
    """A centre equal to a block's `hi` is not a member of it; the next fp32 number inside is."""
    from emu_util import emu_lib
    r, nb = 16, 4
    _, lo, hi = U.tables(r, nb)
    h = float(hi[0])                                                            # upper bound of block x = 0
    inside = float(np.nextafter(np.float32(h), np.float32(-1)))
    fields = {}
    for tag, x in (("at", h), ("inside", inside)):
        scene = _probe_scene(x)
        xyzs, center, scale = U.normalise(scene["xyz"])
        assert torch.equal(xyzs, scene["xyz"]) and float(np.float32(scale)) == 1.0
        (_, occ, _, _) = check_sampled_case(f"probe_{tag}", scene, r, nb, U.all_blocks(nb), emu_lib(), "cpu")
        fields[tag] = occ
    s = r // nb
    block0 = lambda occ: occ[:s, s:2 * s, s:2 * s]                              # block (0, 1, 1): y, z = 0.1 are well inside its bounds
    assert float(block0(fields["at"]).max()) == 0.0                            # the probe is excluded; the anchors are far away
    assert float(block0(fields["inside"]).min()) > 1e-4
    assert float(fields["at"][s:2 * s, s:2 * s, s:2 * s].min()) > 1e-4        # a member of the next block either way
    lo_edge = float(lo[3])
    scene = _probe_scene(lo_edge)
    (_, occ, _, _) = check_sampled_case("probe_lo", scene, r, nb, U.all_blocks(nb), emu_lib(), "cpu")
    assert float(occ[3 * s:, s:2 * s, s:2 * s].max()) == 0.0


def test_scaling_modifier_is_honoured():
    from emu_util import emu_lib
    _, kept = U.golden_scene("r32_nb8")
    blocks = U.sample_blocks(8, 64, 5)
    ref64, counts = U.field_ref64(kept, 32, 8, blocks=blocks, scaling_modifier=0.7)
    e32 = U.e32_of(kept, 32, 8, ref64, blocks=blocks, scaling_modifier=0.7)
    occ = U.make_model(kept, scaling_modifier=0.7).extract_fields(32, 8, lib=emu_lib())
    U.check_field("r32_nb8 modifier 0.7", U.gather_blocks(occ, 8, blocks), ref64, counts, e32)
    plain = U.make_model(kept).extract_fields(32, 8, lib=emu_lib())
    assert float((plain - occ).abs().max()) > 1e-2
    assert torch.equal(U.make_model(kept, scaling_modifier=1.0).extract_fields(32, 8, lib=emu_lib()), plain)


def test_relax_ratio_reaches_the_kernel():
    from dgs_amd import consumers
    from emu_util import emu_lib
    _, kept = U.golden_scene("r32_nb8")
    blocks = U.sample_blocks(8, 32, 6)
    ref64, counts = U.field_ref64(kept, 32, 8, relax_ratio=0.5, blocks=blocks)
    e32 = U.e32_of(kept, 32, 8, ref64, relax_ratio=0.5, blocks=blocks)
    occ = consumers.extract_fields(U.make_model(kept), 32, 8, relax_ratio=0.5, lib=emu_lib())
    U.check_field("r32_nb8 relax 0.5", U.gather_blocks(occ, 8, blocks), ref64, counts, e32)


def test_guards():
    from dgs_amd import _native
    from dgs_amd.denoiser import GaussianModel
    from emu_util import emu_lib
    L = emu_lib()
    _, kept = U.golden_scene("r32_nb8")
    pc = U.make_model(kept)
    with pytest.raises(ValueError):
        pc.extract_fields(36, 8, lib=L)                                          # 36 % 0.25 == 0 but 36 % 8 != 0
    with pytest.raises(AssertionError):
        pc.extract_fields(32, 3, lib=L)                                          # the reference's assert: 32 % (2 / 3) != 0
    empty = GaussianModel(0).set_data(torch.zeros(0, 3), torch.zeros(0, 1, 3), torch.zeros(0, 3), torch.zeros(0, 4), torch.zeros(0, 1))
    with pytest.raises(ValueError):
        empty.extract_fields(32, 8, lib=L)
    assert U.make_model(kept).prune(2.0)._xyz.shape[0] == 0                      # everything pruned: the filters themselves do not raise
    # the C entry point refuses bad shapes and short workspaces
    n = kept["xyz"].shape[0]
    lin, lo, hi = U.tables(32, 8)
    need = L.dgs_gaussian_field_workspace_bytes(n, 8)
    assert need > 48 * n and need % 16 == 0
    assert L.dgs_gaussian_field_workspace_bytes(0, 8) == 0 and L.dgs_gaussian_field_workspace_bytes(n, 0) == 0
    ws, occ = torch.zeros(need, dtype=torch.uint8), torch.zeros(32, 32, 32)
    xyzs = U.normalise(kept["xyz"])[0].contiguous()

    def call(**over):
        a = _native.DgsFieldArgs()
        a.N, a.R, a.nb, a.split, a.mesh_scale, a.scaling_modifier, a.workspace_bytes = n, 32, 8, 4, 1.0, 1.0, need
        a.xyz, a.scaling, a.rotation, a.opacity, a.lin, a.lo, a.hi, a.occ, a.workspace = (
            ctypes.c_void_p(t.data_ptr()) for t in (xyzs, kept["scaling"], kept["rotation"], kept["opacity"], lin, lo, hi, occ, ws))
        for k, v in over.items():
            setattr(a, k, v)
        return L.dgs_gaussian_field(ctypes.byref(a), None)

    assert call() == 0
    for over in (dict(N=0), dict(split=3), dict(R=33), dict(nb=0), dict(workspace_bytes=need - 16), dict(occ=None), dict(lin=None)):
        assert call(**over) == -1, over                                          # DGS_ERR_INVALID_ARGUMENT


def test_abi():
    from dgs_amd import _native
    from emu_util import emu_lib
    inc = os.path.join(ROOT, "include")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgs_field.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_native.FIELD_SYMBOLS) and len(names) == 2
    for lib in (emu_lib(), _native.lib()):
        for n in names:
            assert hasattr(lib, n), n
        assert lib.dgs_abi_version() == _native.ABI_VERSION == 10
    src = '#include <stdio.h>\n#include "dgs_field.h"\nint main(){printf("%zu\\n", sizeof(DgsFieldArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + inc, c, "-o", exe])
        assert ctypes.sizeof(_native.DgsFieldArgs) == int(subprocess.check_output([exe]))
