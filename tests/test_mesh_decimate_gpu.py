"""Mesh decimation on the MI355X (product library): the cases of tests/test_mesh_decimate.py on the device, the 64^3 noise mesh
(801,199 faces: 3,130 blocks of faces for the scan over the block totals, thousands of duplicates for the table), decimate_mesh next to
the steps where F'(n) is not monotone, extract_mesh with a target at R = 64 -- every byte and all five counts against the numpy
restatement of tests/mesh_decimate_util.py."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_decimate_util as D  # noqa: E402
from dgs_amd import _native  # noqa: E402
from test_mesh_decimate import (FIXTURE_RUNS, FIXTURE_STATS, HAND, check, check_decimate_mesh, check_empty, check_extract_mesh,  # noqa: E402
                                check_fixture, check_hand, check_invariance, check_limits)

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", FIXTURE_RUNS)
def test_fixture_on_gpu(name, n):
    check_fixture(DEV, name, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_on_gpu(name):
    check_hand(DEV, name)


@pytest.mark.gpu
def test_empty_meshes_on_gpu():
    check_empty(DEV)


@pytest.mark.gpu
def test_limits_leave_the_rest_untouched_on_gpu():
    check_limits(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("blobs", 16), ("noise24_05", 11)])
def test_invariance_on_gpu(name, n):
    check_invariance(DEV, name, n)


@pytest.mark.gpu
def test_large_noise_mesh_on_gpu():
    """64^3 noise at 0.5, 801,199 faces, at n = 32 (the pinned figures: 19,616 duplicates meet in the table) and at the step where
    F'(n) falls as n grows: F'(63) = 537,821 > F'(64) = 526,857."""
    v, f = D.level_set("noise64_05")
    assert f.shape[0] == 801199
    want = check(DEV, v, f, 32)
    assert tuple(want["counts"][:4]) == FIXTURE_STATS[("noise64_05", 32)] and want["counts"][4] == 0
    L = _native.lib()
    left = {n: D.count_raw(L, v, f, n, DEV)[1] for n in (63, 64)}
    print("noise64_05 F'(63), F'(64)", left)
    assert left == {63: 537821, 64: 526857}
    assert left[63] == D.restatement(v, f, 63)["counts"][1]


@pytest.mark.gpu
def test_decimate_mesh_on_gpu():
    check_decimate_mesh(DEV)


@pytest.mark.gpu
def test_extract_mesh_with_the_decimation_at_r64_on_gpu():
    """The synthetic model of tests/test_mesh_gpu.py (20,000 Gaussians, R = 64, nb = 16)."""
    check_extract_mesh(DEV, "r64_nb16", 5000)


@pytest.mark.gpu
def test_host_synchronisations_on_gpu():
    """cluster_vertices synchronises with the host exactly once (the readback of the counts); decimate_mesh once per count, at most
    eleven times with n_max = 1024."""
    from dgs_amd import consumers
    v, f = D.level_set("noise24_05")
    tv, tf = torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(f.copy()).to(DEV)
    consumers.cluster_vertices(tv, tf, 11)
    consumers.decimate_mesh(tv, tf, 10000)
    torch.cuda.synchronize()
    seen = []
    for fn in (lambda: consumers.cluster_vertices(tv, tf, 11), lambda: consumers.decimate_mesh(tv, tf, 10000)):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        seen.append(len([w for w in caught if "synchroniz" in str(w.message)]))
    assert seen[0] == 1 and 1 <= seen[1] <= 11, seen
