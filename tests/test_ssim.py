"""Fused SSIM loss (csrc/ssim.hip, dgs_amd.losses.ssim / ssim_loss / image_losses, DataParallelTrainer(lambda_ssim=...)) on the
CPU-emulated build of the kernels, against the fp64 restatement of the published formula in tests/ssim_util.py (bounds: there)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ssim_util as U  # noqa: E402

CASES = {
    "noise_16x24": lambda: U.noise_pair((3, 3, 16, 24), 1),
    "odd_37x53": lambda: U.noise_pair((2, 3, 37, 53), 2),
    "one_row_11x40": lambda: U.noise_pair((2, 3, 11, 40), 3),
    "one_channel_48": lambda: U.noise_pair((2, 1, 48, 48), 4),
    "render_like_64": lambda: U.render_like_pair(2, 3, 64, 5),
}


def _leaf(t, device):
    return t.detach().clone().to(device).requires_grad_(True)          # a leaf of its own (on the CPU `.to` alone would alias t)


def check_ssim_case(name, x, y, lib, device, report=None):
    """Values and gradient (non-uniform upstream weights, one of them zero) of losses.ssim; two calls give the same bits."""
    from dgs_amd import losses
    n = x.shape[0]
    wts = torch.linspace(0.3, 1.7, n)
    wts[n // 2] = 0.0
    xd, yd = _leaf(x, device), y.to(device)
    got = losses.ssim(xd, yd, lib=lib)
    (got * wts.to(device)).sum().backward()
    ref64, ref32 = U.ssim_ref(x.double(), y.double()), U.ssim_ref(x, y)
    g64 = U.weighted_grad(lambda t: (U.ssim_ref(t, y.double()) * wts.double()).sum(), x, torch.float64)
    g32 = U.weighted_grad(lambda t: (U.ssim_ref(t, y) * wts).sum(), x, torch.float32)
    vb, ve32 = U.value_bound(ref64, ref32)
    gb, ge32, top = U.grad_bound(g64, g32)
    verr = float((got.detach().cpu().double() - ref64).abs().max())
    gerr = float((xd.grad.cpu().double() - g64).abs().max())
    line = (f"{name}: value err {verr:.3e} (e32 {ve32:.3e}, bound {vb:.3e}); gradient err / max {gerr / top:.3e} "
            f"(e32 {ge32:.3e}, bound {gb / top:.3e})")
    print(line)
    if report is not None:
        report.append(line)
    assert verr <= vb, line
    assert gerr <= gb, line
    assert float(xd.grad.reshape(n, -1)[n // 2].abs().max()) == 0.0            # zero upstream weight: exactly no gradient
    x2 = _leaf(x, device)
    again = losses.ssim(x2, yd, lib=lib)
    (again * wts.to(device)).sum().backward()
    assert torch.equal(again.detach(), got.detach()) and torch.equal(x2.grad, xd.grad)
    return verr, gerr / top


def check_image_losses(name, x, y, b, lib, device, report=None, lambda_mse=0.8, lambda_ssim=0.2):
    """losses.image_losses / ssim_loss on [b, v, C, H, W]: values, the fused gradient of lambda_mse * mse + lambda_ssim * (1 - ssim),
    l2 / psnr against losses.mse_psnr, determinism."""
    from dgs_amd import losses
    x5, y5 = x.reshape(b, -1, *x.shape[1:]), y.reshape(b, -1, *y.shape[1:])
    xd, yd = _leaf(x5, device), y5.to(device)
    loss, l2, psnr, sl = losses.image_losses(xd, yd, lambda_mse, lambda_ssim, lib=lib)
    loss.backward()
    r64, r32 = U.image_loss_ref(x5.double(), y5.double(), lambda_mse, lambda_ssim), U.image_loss_ref(x5, y5, lambda_mse, lambda_ssim)
    for k, (got, i) in {"loss": (loss, 0), "ssim_loss": (sl, 2)}.items():
        vb, e32 = U.value_bound(r64[i], r32[i])
        err = float((got.detach().cpu().double() - r64[i]).abs().max())
        assert err <= vb, (name, k, err, e32, vb)
    only = losses.ssim_loss(xd.detach(), yd, lib=lib)
    assert torch.equal(only, sl.detach())
    assert torch.allclose(l2.detach().cpu().double(), r64[1], rtol=2e-6)
    assert torch.allclose(psnr.cpu().double(), -10.0 * torch.log10(r64[1]), rtol=1e-5, atol=1e-5)
    if x5[0].numel() % 4 == 0:                                                  # dgs_mse_psnr takes samples of a multiple of 4 elements
        _, m_l2, m_psnr = losses.mse_psnr(xd.detach(), yd, lib=lib)
        assert torch.allclose(l2.detach(), m_l2, rtol=2e-6) and torch.allclose(psnr, m_psnr, rtol=1e-5, atol=1e-5)
    g64 = U.weighted_grad(lambda t: U.image_loss_ref(t, y5.double(), lambda_mse, lambda_ssim)[0], x5, torch.float64)
    g32 = U.weighted_grad(lambda t: U.image_loss_ref(t, y5, lambda_mse, lambda_ssim)[0], x5, torch.float32)
    gb, ge32, top = U.grad_bound(g64, g32)
    gerr = float((xd.grad.cpu().double() - g64).abs().max())
    line = f"{name} image_losses: gradient err / max {gerr / top:.3e} (e32 {ge32:.3e}, bound {gb / top:.3e})"
    print(line)
    if report is not None:
        report.append(line)
    assert gerr <= gb, line
    # per-sample outputs carry gradients too: d (sum_b c_b l2_b + d_b ssim_loss_b) / d x through the same single launch
    cw, dw = torch.linspace(0.5, 1.5, b), torch.linspace(2.0, 0.0, b)
    x3 = _leaf(x5, device)
    _, l2b, _, slb = losses.image_losses(x3, yd, lambda_mse, lambda_ssim, lib=lib)
    ((l2b * cw.to(device)).sum() + (slb * dw.to(device)).sum()).backward()
    h64 = U.weighted_grad(lambda t: sum((r * w.double()).sum() for r, w in zip(U.image_loss_ref(t, y5.double(), 0, 0)[1:], (cw, dw))), x5, torch.float64)
    h32 = U.weighted_grad(lambda t: sum((r * w).sum() for r, w in zip(U.image_loss_ref(t, y5, 0, 0)[1:], (cw, dw))), x5, torch.float32)
    hb, _, _ = U.grad_bound(h64, h32)
    assert float((x3.grad.cpu().double() - h64).abs().max()) <= hb
    x2 = _leaf(x5, device)
    again = losses.image_losses(x2, yd, lambda_mse, lambda_ssim, lib=lib)
    again[0].backward()
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(again, (loss, l2, psnr, sl))) and torch.equal(x2.grad, xd.grad)


def check_identical_images(lib, device, shape=(2, 3, 32, 40)):
    """x == y: ssim = 1 within the value bar, and the gradient within the gradient floor of zero (the floor taken against the
    fp64 gradient's max at a perturbed x)."""
    from dgs_amd import losses
    y = torch.rand(shape, generator=torch.Generator().manual_seed(8))
    xd = _leaf(y, device)
    s = losses.ssim(xd, y.to(device), lib=lib)
    s.sum().backward()
    assert float((s.detach().cpu() - 1.0).abs().max()) <= U.VALUE_FLOOR
    pert = y + 0.01 * torch.randn(shape, generator=torch.Generator().manual_seed(9))
    top = float(U.weighted_grad(lambda t: U.ssim_ref(t, y.double()).sum(), pert, torch.float64).abs().max())
    assert float(xd.grad.abs().max()) <= U.GRAD_FLOOR * top, (float(xd.grad.abs().max()), top)


@pytest.mark.parametrize("name", list(CASES))
def test_ssim_values_and_gradient_emulated(name):
    from emu_util import emu_lib
    x, y = CASES[name]()
    check_ssim_case(name, x, y, emu_lib(), torch.device("cpu"))


@pytest.mark.parametrize("name,b", [("noise_16x24", 3), ("odd_37x53", 1), ("render_like_64", 2), ("one_channel_48", 2)])
def test_image_losses_emulated(name, b):
    from emu_util import emu_lib
    x, y = CASES[name]()
    check_image_losses(name, x, y, b, emu_lib(), torch.device("cpu"))


def test_ssim_accepts_five_dimensions_and_other_data_ranges():
    from dgs_amd import losses
    from emu_util import emu_lib
    x, y = U.noise_pair((2, 2, 3, 16, 24), 6)
    s5 = losses.ssim(x, y, lib=emu_lib())
    assert s5.shape == (4,) and torch.equal(s5, losses.ssim(x.flatten(0, 1), y.flatten(0, 1), lib=emu_lib()))
    x4, y4 = (x * 255.0).flatten(0, 1), (y * 255.0).flatten(0, 1)
    ref64, ref32 = U.ssim_ref(x4.double(), y4.double(), 255.0), U.ssim_ref(x4, y4, 255.0)
    assert float((losses.ssim(x4, y4, data_range=255.0, lib=emu_lib()).double() - ref64).abs().max()) <= U.value_bound(ref64, ref32)[0]


def test_identical_images_emulated():
    from emu_util import emu_lib
    check_identical_images(emu_lib(), torch.device("cpu"))


def test_planes_smaller_than_the_window_are_refused():
    from dgs_amd import _native, losses
    from emu_util import emu_lib
    x = torch.rand(1, 3, 10, 32)
    with pytest.raises(ValueError):
        losses.ssim(x, x.clone(), lib=emu_lib())
    with pytest.raises(ValueError):
        losses.image_losses(torch.rand(1, 1, 3, 32, 10), torch.rand(1, 1, 3, 32, 10), lib=emu_lib())
    out, ws = torch.zeros(1), torch.zeros(64)
    a = _native.DgsSsimArgs()
    a.N, a.C, a.H, a.W, a.B, a.data_range = 1, 3, 10, 32, 1, 1.0
    a.x, a.y, a.ssim, a.workspace = (ctypes.c_void_p(t.data_ptr()) for t in (x, x, out, ws))
    assert emu_lib().dgs_ssim(ctypes.byref(a), None) == -1                      # DGS_ERR_INVALID_ARGUMENT
    a.g, a.dx, a.saved = (ctypes.c_void_p(t.data_ptr()) for t in (out, torch.zeros_like(x), torch.zeros(3 * x.numel())))
    assert emu_lib().dgs_ssim_backward(ctypes.byref(a), None) == -1
    assert emu_lib().dgs_status_string(-1).decode().startswith("invalid argument")
    assert emu_lib().dgs_ssim_workspace_floats(1, 3, 10, 32) == 0 and emu_lib().dgs_ssim_saved_floats(1, 3, 32, 10) == 0


def test_ctypes_struct_matches_c_layout():
    from dgs_amd import _native
    src = '#include <stdio.h>\n#include "dgs_loss.h"\nint main(){printf("%zu\\n", sizeof(DgsSsimArgs));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe])
        assert ctypes.sizeof(_native.DgsSsimArgs) == int(subprocess.check_output([exe]))


def _trainer_params(lambda_ssim, lr=0.05):
    """One DataParallelTrainer step (width 256, one layer, 16^2 views, emulator library, a world of one, SGD) -> parameters, trainer."""
    from dgs_amd import denoiser as dn
    from dgs_amd.train import DataParallelTrainer
    from dit_util import synth_inputs
    from emu_util import emu_lib
    from oracle import dit_oracle as D
    cfg = D.Cfg(width=256, num_layers=1)
    m = dn.DGSDenoiser(dict(width=256, in_channels=9, patch_size=8, num_layers=1), device="cpu", lib=emu_lib())
    m.reset_parameters(seed=1)
    images, ray_o, ray_d, t, c2w, k = synth_inputs(cfg, 2, 2, 16, seed=9)
    batch = dict(image=images, ray_o=ray_o, ray_d=ray_d, c2w=c2w, fxfycxcy=k)
    target = torch.rand(2, 2, 3, 16, 16, generator=torch.Generator().manual_seed(3))
    kw = {} if lambda_ssim == "absent" else dict(lambda_ssim=lambda_ssim)
    with DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=lr), bucket_bytes=1 << 20, **kw) as tr:
        loss = tr.step(batch, t, target)
        return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone(), float(loss), tr


def test_trainer_takes_the_ssim_term_only_when_asked():
    from dgs_amd import denoiser as dn
    m0 = dn.DGSDenoiser(dict(width=256, in_channels=9, patch_size=8, num_layers=1), device="cpu")
    m0.reset_parameters(seed=1)
    start = torch.cat([p.detach().reshape(-1) for p in m0.parameters()])
    absent, loss_absent, tr = _trainer_params("absent")
    assert tr.last_ssim_loss is None and tr.lambda_ssim is None
    assert not torch.equal(absent, start)                                       # the step moved the parameters (lr != 0)
    none, loss_none, _ = _trainer_params(None)
    assert torch.equal(none, absent) and loss_none == loss_absent               # lambda_ssim=None is today's path, bit for bit
    zero, loss_zero, tr0 = _trainer_params(0.0)
    assert tr0.last_ssim_loss.shape == (2,) and bool(torch.isfinite(tr0.last_ssim_loss).all()) and not tr0.last_ssim_loss.requires_grad
    assert torch.allclose(zero, none, rtol=1e-5)                                # the MSE part of the fused gradient: same expression, another kernel
    assert abs(loss_zero - loss_none) <= 2e-6 * abs(loss_none)
    a, loss_a, tra = _trainer_params(0.2)
    b, loss_b, _ = _trainer_params(0.2)
    assert not torch.equal(a, none) and loss_a > loss_none
    assert torch.equal(a, b) and loss_a == loss_b
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(tra.last_ssim_loss).all())
