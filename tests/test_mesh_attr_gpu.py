"""Mesh attributes on the MI355X (product library): the cases of tests/test_mesh_attr.py on the device, the whole level set of the
r64_nb16 scene (20,000 Gaussians, R = 64: 80,096 vertices, up to 2,385 members a point), and the host synchronisations
of the Python call -- against the fp64 restatement and the bars of tests/mesh_attr_util.py."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import field_util as FU  # noqa: E402
import mesh_attr_util as M  # noqa: E402
from test_mesh_attr import (check_arguments, check_blobs, check_crowded, check_defaults_unchanged, check_edges, check_extract_mesh,  # noqa: E402
                            check_fixture, check_invariance, check_sphere, check_trivial)

DEV = "cuda:0"


@pytest.mark.gpu
def test_trivial_sizes_on_gpu():
    check_trivial(DEV)


@pytest.mark.gpu
def test_sphere_on_gpu():
    check_sphere(DEV)


@pytest.mark.gpu
def test_three_blobs_on_gpu():
    check_blobs(DEV)


@pytest.mark.gpu
def test_crowded_cells_on_gpu():
    check_crowded(DEV)


@pytest.mark.gpu
def test_window_edges_on_gpu():
    check_edges(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name,filtered", [("r32_nb8", False), ("r32_nb8", True), ("r40_nb4", False), ("r40_nb4", True)])
def test_fixture_scene_on_gpu(name, filtered):
    check_fixture(DEV, name, filtered)


@pytest.mark.gpu
def test_large_scene_on_gpu():
    """r64_nb16: 20,000 Gaussians (about 17,000 after the pipeline's filters), the whole level set at R = 64."""
    got = check_fixture(DEV, "r64_nb16", False)
    assert got["density"].shape[0] > 10000


@pytest.mark.gpu
def test_extract_mesh_with_attributes_on_gpu():
    check_extract_mesh(DEV)
    check_extract_mesh(DEV, "r64_nb16")


@pytest.mark.gpu
def test_invariance_on_gpu():
    check_invariance(DEV)


@pytest.mark.gpu
def test_argument_checks_on_gpu():
    check_arguments(DEV)


@pytest.mark.gpu
def test_defaults_unchanged_on_gpu():
    check_defaults_unchanged(DEV)


@pytest.mark.gpu
def test_host_synchronisations_on_gpu():
    """mesh_attributes is one C call on the current stream; the only synchronisation with the host is the normalisation's .item()."""
    from dgs_amd import consumers
    pc = FU.make_model(FU.golden_scene("r32_nb8")[1], DEV)
    pts = M.random_points(1000, 7, 0.7).to(DEV)
    consumers.mesh_attributes(pc, pts, num_blocks=8)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            consumers.mesh_attributes(pc, pts, num_blocks=8, want=("colors", "normals", "density"))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    seen = [str(w.message) for w in caught if "synchroniz" in str(w.message)]
    assert len(seen) <= 1, seen                                              # pc.mesh_scale = ....item(), as in extract_fields
