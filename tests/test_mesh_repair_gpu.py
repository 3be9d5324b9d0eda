"""Mesh repair on the MI355X (product library): the cases of tests/test_mesh_repair.py on the device, the 64^3 noise mesh clustered
to about 10^5 faces (more than 87,381 faces: the first size at which a thread of the one-workgroup scan takes two blocks of corners),
extract_mesh with the repair at R = 64, the host synchronisations -- every byte and all ten counts against the numpy restatement of
tests/mesh_repair_util.py, the census against the restated census."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_repair_util as R  # noqa: E402
from test_mesh_repair import CASES, check, check_case, check_empty, check_extract_mesh, check_slab  # noqa: E402

DEV = "cuda:0"
NOISE_N = 26                                                                  # cells per axis: 801,199 faces -> 98,688


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_case_on_gpu(name):
    check_case(DEV, name)


@pytest.mark.gpu
def test_clustered_noise_mesh_on_gpu():
    """64^3 noise at 0.5 through cluster_vertices: the kind of mesh the decimation hands to the repair, at the pipeline's face count."""
    from dgs_amd import consumers
    v, f = R.level_set("noise64_05")
    cv, cf = consumers.cluster_vertices(torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(f.copy()).to(DEV), NOISE_N)
    assert cf.shape[0] == 98688 and 3 * cf.shape[0] > 1024 * 256, cf.shape      # more blocks of corners than the last scan has threads
    want, before = check(DEV, cv.cpu().numpy(), cf.cpu().numpy())
    print("clustered noise", tuple(cf.shape), "census", before, "counts", want["counts"])
    assert before["non_manifold_edges"] > 0 and before["non_manifold_vertices"] > 0


@pytest.mark.gpu
def test_empty_meshes_on_gpu():
    check_empty(DEV)


@pytest.mark.gpu
def test_clustered_slab_on_gpu():
    check_slab(DEV)


@pytest.mark.gpu
def test_extract_mesh_with_the_repair_at_r64_on_gpu():
    """The synthetic model of tests/test_mesh_gpu.py (20,000 Gaussians, R = 64, nb = 16)."""
    check_extract_mesh(DEV, "r64_nb16", 5000)


@pytest.mark.gpu
def test_host_synchronisations_on_gpu():
    """repair_mesh synchronises with the host exactly once (the readback of the ten counts), mesh_topology once (its seven numbers)."""
    from dgs_amd import consumers
    v, f = R.tetrahedra_on_a_vertex(300)
    tv, tf = torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(f.copy()).to(DEV)
    consumers.repair_mesh(tv, tf)
    consumers.mesh_topology(tv, tf)
    torch.cuda.synchronize()
    seen = []
    for fn in (lambda: consumers.repair_mesh(tv, tf), lambda: consumers.repair_mesh(tv, tf, return_counts=True), lambda: consumers.mesh_topology(tv, tf)):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        seen.append(len([w for w in caught if "synchroniz" in str(w.message)]))
    assert seen == [1, 1, 1], seen
