"""Mesh clean-up on the MI355X (product library): the cases of tests/test_mesh_clean.py on the device, two meshes of 64^3 noise large
enough for contention on one root and for scans over many blocks, extract_mesh with the clean-up at R = 64, and a .ply round trip --
every byte and all five counts against the numpy restatement of tests/mesh_clean_util.py."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_clean_util as C  # noqa: E402
from test_mesh_clean import (FIXTURE_RUNS, HAND, check, check_empty, check_extract_mesh, check_fixture, check_hand, check_limits,  # noqa: E402
                             check_ply_round_trip)

DEV = "cuda:0"
# name -> (faces, components) of the restatement
LARGE = {"noise64_05": (801199, 2615), "noise64_08": (395359, 22576)}


@pytest.mark.gpu
@pytest.mark.parametrize("name,min_f,min_d", FIXTURE_RUNS)
def test_fixture_on_gpu(name, min_f, min_d):
    check_fixture(DEV, name, min_f, min_d)


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
@pytest.mark.parametrize("name,min_f,min_d,kept", [("noise64_05", 64, 20.0, 1), ("noise64_08", 64, 20.0, 0), ("noise64_08", 64, 0.0, 965)])
def test_large_noise_mesh_on_gpu(name, min_f, min_d, kept):
    """64^3 noise at 0.5: one giant component among thousands (every face of it adds to one counter, the block totals of 3,130 blocks
    are scanned); at 0.8: 22,576 components (several labels in most waves), none of which reaches a fifth of the mesh's diagonal and
    965 of which have 64 faces or more."""
    v, f = C.level_set(name)
    comp = C.level_set_components(name)
    assert (f.shape[0], comp["roots"].shape[0]) == LARGE[name]
    if name == "noise64_05":
        assert comp["n"].max() > 0.9 * f.shape[0]
    want = check(DEV, v, f, min_f, min_d, comp)
    print(name, "V", v.shape[0], "F", f.shape[0], "counts", want["counts"])
    assert want["counts"][2:] == [LARGE[name][1], kept, 0]


@pytest.mark.gpu
def test_extract_mesh_with_the_clean_up_at_r64_on_gpu():
    """The synthetic model of tests/test_mesh_gpu.py (20,000 Gaussians, R = 64, nb = 16)."""
    check_extract_mesh(DEV, "r64_nb16")


@pytest.mark.gpu
def test_ply_round_trip_on_gpu():
    check_ply_round_trip(DEV)


@pytest.mark.gpu
def test_one_host_synchronisation_on_gpu():
    """remove_small_components synchronises with the host exactly once (the readback of the counts)."""
    from dgs_amd import consumers
    v, f = C.level_set("noise24_05")
    tv, tf = torch.from_numpy(v.copy()).to(DEV), torch.from_numpy(f.copy()).to(DEV)
    consumers.remove_small_components(tv, tf)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            consumers.remove_small_components(tv, tf)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in caught]
