"""Mesh smoothing on the MI355X (product library): the cases of tests/test_mesh_smooth.py on the device, the 64^3 noise mesh (801,199
faces, 1,512 blocks of vertices for the scan over the block totals) at 2 iterations, extract_mesh with the smoothing at R = 64, the
host synchronisations -- every byte and all four counts against the numpy restatement of tests/mesh_smooth_util.py."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_smooth_util as S  # noqa: E402
from test_mesh_smooth import CASES, check, check_case, check_empty, check_extract_mesh, check_invariance, check_smooths  # noqa: E402

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_case_on_gpu(name):
    check_case(DEV, name)


@pytest.mark.gpu
def test_large_noise_mesh_on_gpu():
    """64^3 noise at 0.5, 801,199 faces, 2 iterations."""
    v, f = S.level_set("noise64_05")
    assert f.shape[0] == 801199
    want = check(DEV, v, f, iterations=2)
    assert want["counts"] == [0, 0, 0, 0]


@pytest.mark.gpu
def test_empty_meshes_on_gpu():
    check_empty(DEV)


@pytest.mark.gpu
def test_invariance_on_gpu():
    check_invariance(DEV)


@pytest.mark.gpu
def test_smooths_without_shrinking_on_gpu():
    check_smooths(DEV)


@pytest.mark.gpu
def test_extract_mesh_with_the_smoothing_at_r64_on_gpu():
    """The synthetic model of tests/test_mesh_gpu.py (20,000 Gaussians, R = 64, nb = 16)."""
    check_extract_mesh(DEV, "r64_nb16", 5000)


@pytest.mark.gpu
def test_host_synchronisations_on_gpu():
    """smooth_mesh does not synchronise with the host; with return_counts=True exactly once (the readback of the counts)."""
    from dgs_amd import consumers
    v, f = S.level_set("noise24_05")
    tv, tf = torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(f.copy()).to(DEV)
    consumers.smooth_mesh(tv, tf)
    consumers.smooth_mesh(tv, tf, return_counts=True)
    torch.cuda.synchronize()
    seen = []
    for fn in (lambda: consumers.smooth_mesh(tv, tf), lambda: consumers.smooth_mesh(tv, tf, return_counts=True)):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        seen.append(len([w for w in caught if "synchroniz" in str(w.message)]))
    assert seen == [0, 1], seen
