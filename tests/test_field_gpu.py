"""Gaussian density field on the MI355X (product library): the fixture cases of tests/test_field.py, the pipeline's setting
R = 256, nb = 64 on 262,144 Gaussians, split 8, and one run from a denoiser's output -- against tests/golden/field_ref.npz and the
fp64 restatement of tests/field_util.py only.  DGS_FIELD_PARITY=<file> appends the measured deviations of each case
(profiles/field_parity.txt comes from it)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import field_util as U  # noqa: E402
from test_field import check_fixture_case, check_sampled_case  # noqa: E402


def _report(lines):
    path = os.environ.get("DGS_FIELD_PARITY")
    if path:
        with open(path, "a") as f:
            f.write("".join(ln + "\n" for ln in lines))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(U.FIXTURE_CASES))
def test_field_matches_the_reference_on_gpu(name):
    lines = []
    check_fixture_case(name, None, "cuda:0", lines)
    _report(lines)


def _blocks_around(scene, r, nb, count, seed):
    """`count` distinct blocks: half of them the blocks that hold the centres of seeded Gaussians (non-empty by construction), the
    rest drawn from the whole grid."""
    xyzs = U.normalise(scene["xyz"])[0]
    g = torch.Generator().manual_seed(seed)
    pick = torch.randperm(xyzs.shape[0], generator=g)[:4 * count]
    voxel = ((xyzs[pick].double() + 1) / 2 * (r - 1)).round().clamp(0, r - 1).long() // (r // nb)
    near = []
    for b in voxel.tolist():
        if tuple(b) not in near:
            near.append(tuple(b))
        if len(near) == count // 2:
            break
    rest = [b for b in U.sample_blocks(nb, count, seed) if b not in near][:count - len(near)]
    return near + rest


@pytest.mark.gpu
def test_field_at_the_pipeline_setting_on_gpu():
    """R = 256, nb = 64 (one wave per block), N = 262,144 on the shell: 512 sampled blocks, at least half of them non-empty."""
    scene = U.make_scene(262144, 21)
    blocks = _blocks_around(scene, 256, 64, 512, 22)
    assert len(blocks) == len(set(blocks)) == 512
    lines = []
    check_sampled_case("pipeline_r256_nb64_n262144", scene, 256, 64, blocks, None, "cuda:0", lines, min_nonempty=256)
    _report(lines)


@pytest.mark.gpu
def test_field_split_eight_on_gpu():
    """R = 128, nb = 16: 512 voxels per block, two per thread in one pass."""
    scene = U.make_scene(20000, 23)
    blocks = _blocks_around(scene, 128, 16, 48, 24)
    lines = []
    check_sampled_case("r128_nb16_n20000", scene, 128, 16, blocks, None, "cuda:0", lines, min_nonempty=24)
    _report(lines)


@pytest.mark.gpu
def test_denoiser_output_through_filters_and_field_on_gpu():
    """DGSDenoiser (width 1024, two layers, 64^2 views, random weights) -> prepare_to_save -> apply_all_filters -> extract_fields(64, 16)."""
    from dgs_amd import denoiser as dn
    from dgs_amd import synth
    dev = torch.device("cuda:0")
    batch, t = synth.make_batch(1, 64, V=4, device=dev, seed=5, with_t=True)
    m = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=2), device=dev)
    m.reset_parameters(seed=2)
    m = m.to(dev)
    m.eval()
    with torch.no_grad():
        _, models = m(batch, t)
    pc = models[0]
    n = pc._xyz.shape[0]
    assert pc.apply_all_filters(**U.PIPELINE_FILTERS) is pc
    if pc._xyz.shape[0] < 16:                                     # random weights: should the pipeline's thresholds leave too little,
        _, models = m(batch, t)                                   # filter by opacity alone
        pc = models[0].apply_all_filters(opacity_thres=0.0, crop_bbx=None)
    assert 16 <= pc._xyz.shape[0] <= n
    occ = pc.extract_fields(64, 16)
    assert occ.shape == (64, 64, 64) and occ.dtype == torch.float32 and occ.is_cuda
    assert bool(torch.isfinite(occ).all()) and float(occ.max()) > 0
    assert pc.mesh_center.shape == (3,) and pc.mesh_scale > 0
    assert torch.equal(pc.extract_fields(64, 16), occ)
