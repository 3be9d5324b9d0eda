"""Depth and alpha maps of the rasterizer (forward_views(aux=True), backward_views(grad_depth=, grad_alpha=)) on the CPU emulator against
the oracle, through the identity of raster_aux_util: the aux forms of blend_forward_kernel (list and scan forms, both exponentials), of
blend_backward_kernel (atomic and deterministic), the tenth sum's way through flush / slots / gather, and the z row of the preprocess
backward."""
import functools

import numpy as np
import pytest
import torch

import raster_aux_util as A
from emu_util import emu_backend
from util_scene import small_scene

DEV = torch.device("cpu")

# P, H, W, views, SH degree, background, seed, log_scale   (the scenes of test_raster_backward_emu.py)
SCENES = {
    "partial_tiles": (200, 40, 56, 1, 0, (1.0, 1.0, 1.0), 1, -2.6),
    "two_views_sh3": (200, 33, 17, 2, 3, (1.0, 1.0, 1.0), 3, -2.6),
    "three_views_bg": (200, 48, 48, 3, 1, (0.3, 0.6, 0.9), 5, -2.6),
    "long_lists": (1500, 32, 32, 1, 0, (1.0, 1.0, 1.0), 4, -1.5),          # several 256-entry rounds per tile
}


@functools.lru_cache(maxsize=None)
def reference(name):
    P, H, W, views, deg, bg, seed, log_scale = SCENES[name]
    sc, cams = small_scene(P, W, H, seed=seed, sh_degree=deg, n_views=views, log_scale=log_scale)
    return A.AuxReference(sc, cams, H, W, bg=bg, sh_degree=deg, seed=seed)


@pytest.fixture(params=["atomic", "deterministic"])
def backward_form(request):
    """Both forms of the backward (dgs_raster.h `scratch`), as tests/test_raster_backward_emu.py parametrises them."""
    be = emu_backend()
    old = be.deterministic
    be.deterministic = request.param == "deterministic"
    be.last_backward_deterministic = None
    yield request.param
    assert be.last_backward_deterministic in (None, request.param == "deterministic")
    be.deterministic = old


@pytest.mark.parametrize("exact", [True, False], ids=["exact_exp", "product_default"])
@pytest.mark.parametrize("name", list(SCENES))
def test_maps_and_gradients_match_oracle(name, exact, backward_form):
    ref = reference(name)
    st = A.assert_aux_parity(emu_backend(), ref, DEV, exact, what=f"{name} {backward_form}")
    if name == "long_lists":
        assert float(st[7].max()) > 0.999          # some pixel terminated (T < 1e-4): the maps stop where the colour stops


@pytest.mark.parametrize("form", [1, 2, 3])
def test_every_binning_form(form, monkeypatch):
    """Instance list + rank sort, per-tile scan (blend_forward_kernel<SCAN = true>), instance list + LDS sort: the same maps."""
    monkeypatch.setenv("DGS_RASTER_BIN", str(form))
    ref = reference("three_views_bg")
    for exact in (True, False):
        st = A.forward(emu_backend(), ref, DEV, exact=exact, aux=True)
        A.assert_maps(ref, st[6], st[7], exact, what=f"binning form {form}")


def test_absent_gradient_is_zero_gradient(backward_form):
    A.case_absent_gradient_is_zero_gradient(emu_backend(), reference("three_views_bg"), DEV, bitwise=True)


@pytest.mark.parametrize("exact", [True, False], ids=["exact_exp", "product_default"])
def test_aux_off_is_the_call_that_never_heard_of_aux(exact, backward_form):
    A.case_aux_off_is_the_call_that_never_heard_of_aux(emu_backend(), reference("two_views_sh3"), DEV, exact, bitwise=True)


def test_deterministic_form_is_bit_reproducible():
    A.case_deterministic_form_is_bit_reproducible(emu_backend(), reference("long_lists"), DEV)


def test_one_map_alone_is_refused():
    """The C ABI takes both maps or neither (P = 0: the call only fills its outputs, so nothing else of the block matters)."""
    import ctypes
    from dgs_amd import _native
    cb = _native.ALLOC_FN(lambda n, u: 0)
    col, dep, alp = torch.ones(3 * 256), torch.ones(256), torch.ones(256)

    def call(depth, alpha):
        a = _native.DgsRasterForwardArgs()
        a.P, a.width, a.height, a.V, a.views_per_set = 0, 16, 16, 1, 1
        a.out_color, a.geom_alloc, a.img_alloc, a.binning_alloc = col.data_ptr(), cb, cb, cb
        a.out_depth, a.out_alpha = depth, alpha
        return emu_backend().lib.dgs_raster_forward(ctypes.byref(a), None)

    assert call(dep.data_ptr(), None) == -1 and call(None, alp.data_ptr()) == -1          # DGS_ERR_INVALID_ARGUMENT
    assert float(dep.min()) == 1.0
    assert call(dep.data_ptr(), alp.data_ptr()) == 0 and call(None, None) == 0
    assert float(dep.abs().max()) == 0.0 and float(alp.abs().max()) == 0.0 and float(col.abs().max()) == 0.0


def test_scratch_size_of_an_aux_call():
    lib = emu_backend().lib
    plain = lib.dgs_raster_backward_scratch_bytes(1000, 64, 64, 2, 100000)
    aux = lib.dgs_raster_backward_aux_scratch_bytes(1000, 64, 64, 2, 100000)
    assert 4 * 100000 <= aux - plain <= 4 * 100000 + 512          # four bytes per instance slot (+ the carve's alignment)


def test_autograd_three_outputs_match_dropin_binding_with_torch_activations(backward_form):
    import dgs_amd.raster as R
    R._default = emu_backend()                       # the binding's `_C` resolves the backend lazily
    A.case_autograd_three_outputs(emu_backend(), DEV, what=backward_form)


def test_autograd_unused_maps_change_nothing():
    A.case_autograd_unused_maps(emu_backend(), DEV, bitwise=True)


def test_renderer_return_aux(backward_form):
    """Renderer.forward(return_aux=True) and its backward at 32^2 (the 256^2 case runs on the device)."""
    A.case_renderer_return_aux(emu_backend(), DEV, 32, 2, what=f"renderer 32 {backward_form}")
