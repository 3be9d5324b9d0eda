"""Marching cubes on the MI355X (product library): the cases of tests/test_mesh.py bit for bit against the restatement of
tests/mesh_util.py, the pipeline's setting R = 256, nb = 64 on 262,144 Gaussians checked with torch ops on the device, and one run from
a denoiser's output to a .ply file."""
import os
import sys
import tempfile
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import field_util as FU  # noqa: E402
import mesh_util as U  # noqa: E402
from test_mesh import NAMED, check_limits, check_named_case, check_pipeline_case  # noqa: E402


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NAMED))
def test_mesh_matches_the_restatement_on_gpu(name):
    """A vertex that differs in its last bit here would be a finding about the division flags of mesh.hip, not a tolerance to widen."""
    check_named_case(name, None, "cuda:0")


@pytest.mark.gpu
def test_limits_leave_the_rest_untouched_on_gpu():
    from dgs_amd import _native
    check_limits(_native.lib(), "cuda:0")


@pytest.mark.gpu
def test_extract_mesh_against_the_restatement_at_r64_on_gpu():
    """apply_all_filters -> extract_mesh(R = 64, nb = 16) on 20,000 Gaussians: every vertex and triangle against the restatement applied
    to the device's own field."""
    check_pipeline_case("r64_nb16", None, "cuda:0")


def _device_checks(occ, level, vertices, faces):
    """The table-independent checks with torch ops on the device: V = crossings, every directed edge once, its reverse once unless
    both ends lie on the same boundary face, no unreferenced vertex, no repeated index.  -> (open edges, crossings)."""
    lv = torch.tensor(level, dtype=torch.float32, device=occ.device)
    assert not bool((occ == lv).any())
    ins = occ > lv
    crossings = int((ins[:-1] != ins[1:]).sum()) + int((ins[:, :-1] != ins[:, 1:]).sum()) + int((ins[:, :, :-1] != ins[:, :, 1:]).sum())
    V = vertices.shape[0]
    assert V == crossings
    t = faces.long()
    assert bool((t >= 0).all()) and bool((t < V).all())
    assert not bool(((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).any())
    assert torch.unique(t).numel() == V
    d = torch.cat((t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]))
    key = d[:, 0] * V + d[:, 1]
    uniq = torch.unique(key)
    assert uniq.numel() == key.numel()                                      # no directed edge twice
    lonely = ~torch.isin(d[:, 1] * V + d[:, 0], uniq)
    top = torch.tensor([s - 1 for s in occ.shape], dtype=torch.float32, device=occ.device)
    on_face = torch.cat((vertices == 0, vertices == top[None]), dim=1)      # [V, 6]
    same_face = (on_face[d[lonely, 0]] & on_face[d[lonely, 1]]).any(dim=1)
    assert bool(same_face.all())                                            # an edge without a partner lies in the grid's boundary
    return int(lonely.sum()), crossings


@pytest.mark.gpu
def test_mesh_at_the_pipeline_setting_on_gpu():
    """R = 256, nb = 64, N = 262,144: extract_mesh with its defaults, twice; marching_cubes on the same field in index coordinates."""
    from dgs_amd import consumers
    pc = FU.make_model(FU.make_scene(262144, 21), "cuda:0")
    mesh = pc.extract_mesh()
    again = pc.extract_mesh()
    assert torch.equal(mesh.vertices, again.vertices) and torch.equal(mesh.faces, again.faces)
    occ = pc.extract_fields(256, 64)
    v, t = consumers.marching_cubes(occ, 0.005)
    assert v.shape[0] > 10000 and t.shape[0] > 10000
    assert torch.equal(mesh.faces, t) and torch.equal(mesh.vertices, v / 255.0 * 2 - 1)
    assert float(mesh.vertices.min()) >= -1.0 and float(mesh.vertices.max()) <= 1.0
    n_open, crossings = _device_checks(occ, 0.005, v, t)
    print(f"pipeline setting: V {v.shape[0]} F {t.shape[0]} crossings {crossings} open (boundary) edges {n_open}")


@pytest.mark.gpu
def test_denoiser_output_to_a_mesh_file_on_gpu():
    """DGSDenoiser (width 1024, two layers, 64^2 views, random weights) -> apply_all_filters -> extract_mesh -> save_mesh_ply; and
    marching_cubes synchronises with the host exactly once (the {V, F} readback)."""
    from dgs_amd import consumers
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
    pc = models[0].apply_all_filters(opacity_thres=0.0, crop_bbx=None)
    occ = pc.extract_fields(64, 16)
    level = 0.5 * float(occ.max())                                          # random weights: a level the field certainly crosses
    assert level > 0
    mesh = pc.extract_mesh(level, 64, 16)
    assert mesh.vertices.is_cuda and mesh.faces.is_cuda and mesh.vertices.shape[0] >= 4 and mesh.faces.shape[0] >= 4
    v, f = consumers.marching_cubes(occ, level)
    _device_checks(occ, level, v, f)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mesh.ply")
        consumers.save_mesh_ply(path, mesh.vertices, mesh.faces)
        v2, f2 = consumers.load_mesh_ply(path)
    assert np.array_equal(v2, mesh.vertices.cpu().numpy()) and np.array_equal(f2, mesh.faces.cpu().numpy())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            consumers.marching_cubes(occ, level)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in caught]
