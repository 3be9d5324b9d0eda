"""Depth and alpha maps of the rasterizer on MI355X: the cases of tests/test_raster_aux_emu.py on the device (the oracle identity of
raster_aux_util: maps by parity_util's forward rule scaled by the map's max, gradients at 2e-4 of each tensor's max), a DiffusionGS-shaped
scene, and the 256^2 trained-like scene through Renderer.forward(return_aux=True) and its backward."""
import functools

import numpy as np
import pytest
import torch

import raster_aux_util as A
from dgs_amd import synth
from util_scene import small_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# P, H, W, views, SH degree, background, seed, log_scale
SCENES = {
    "partial_tiles": (200, 40, 56, 1, 0, (1.0, 1.0, 1.0), 1, -2.6),
    "two_views_sh3": (200, 33, 17, 2, 3, (1.0, 1.0, 1.0), 3, -2.6),
    "three_views_bg": (200, 48, 48, 3, 1, (0.3, 0.6, 0.9), 5, -2.6),
    "long_lists": (1500, 32, 32, 1, 0, (1.0, 1.0, 1.0), 4, -1.5),          # several 256-entry rounds per tile
}


@functools.lru_cache(maxsize=None)
def reference(name):
    if name == "diffusiongs_64":
        sc = synth.gaussian_scene(64, regime="trained", seed=0)
        cams, _, _ = synth.render_cameras(64, 4, phase_deg=10)
        return A.AuxReference(sc, cams, 64, 64)
    P, H, W, views, deg, bg, seed, log_scale = SCENES[name]
    sc, cams = small_scene(P, W, H, seed=seed, sh_degree=deg, n_views=views, log_scale=log_scale)
    return A.AuxReference(sc, cams, H, W, bg=bg, sh_degree=deg, seed=seed)


def _backend():
    from dgs_amd.raster import default_backend
    return default_backend()


@pytest.fixture(autouse=True)
def poisoned_lds():
    """Every test starts from LDS full of NaN patterns, as in tests/test_raster_backward_gpu.py: the aux forms stage a wider record
    (x, y, z, -) and multiply masked-out lanes' z by a zero weight, so a slot nothing was staged into must hold finite words."""
    from dgs_amd.dit import DitOps
    DitOps().poison_lds()
    yield


@pytest.fixture(params=["atomic", "deterministic"])
def backward_form(request):
    be = _backend()
    old = be.deterministic
    be.deterministic = request.param == "deterministic"
    be.last_backward_deterministic = None
    yield request.param
    assert be.last_backward_deterministic in (None, request.param == "deterministic")
    be.deterministic = old


@pytest.mark.parametrize("exact", [True, False], ids=["exact_exp", "product_default"])
@pytest.mark.parametrize("name", list(SCENES) + ["diffusiongs_64"])
def test_maps_and_gradients_match_oracle(name, exact, backward_form):
    st = A.assert_aux_parity(_backend(), reference(name), DEV, exact, what=f"gpu {name} {backward_form}")
    if name == "long_lists":
        assert float(st[7].max()) > 0.999          # some pixel terminated (T < 1e-4)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_every_binning_form(form, monkeypatch):
    monkeypatch.setenv("DGS_RASTER_BIN", str(form))
    ref = reference("three_views_bg")
    for exact in (True, False):
        st = A.forward(_backend(), ref, DEV, exact=exact, aux=True)
        A.assert_maps(ref, st[6], st[7], exact, what=f"gpu binning form {form}")


def test_absent_gradient_is_zero_gradient(backward_form):
    A.case_absent_gradient_is_zero_gradient(_backend(), reference("three_views_bg"), DEV, bitwise=backward_form == "deterministic")


@pytest.mark.parametrize("exact", [True, False], ids=["exact_exp", "product_default"])
def test_aux_off_is_the_call_that_never_heard_of_aux(exact, backward_form):
    A.case_aux_off_is_the_call_that_never_heard_of_aux(_backend(), reference("two_views_sh3"), DEV, exact, bitwise=backward_form == "deterministic")


def test_deterministic_form_is_bit_reproducible():
    A.case_deterministic_form_is_bit_reproducible(_backend(), reference("long_lists"), DEV)
    A.case_deterministic_form_is_bit_reproducible(_backend(), reference("diffusiongs_64"), DEV)


def test_autograd_three_outputs_match_dropin_binding_with_torch_activations(backward_form):
    A.case_autograd_three_outputs(_backend(), DEV, what=f"gpu {backward_form}")


def test_autograd_unused_maps_change_nothing(backward_form):
    A.case_autograd_unused_maps(_backend(), DEV, bitwise=backward_form == "deterministic")


def test_renderer_return_aux_256():
    """256^2, P = 262,146, trained-like, 2 views, through Renderer.forward(return_aux=True) and its backward."""
    A.case_renderer_return_aux(_backend(), DEV, 256, 2, what="gpu renderer 256")
