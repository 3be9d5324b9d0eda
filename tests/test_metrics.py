"""dgs_amd.metrics: MetricComputer's PSNR and SSIM on the CPU-emulated build of the kernels, against the reference's expressions.
The checks are functions of a device; tests/test_lpips_gpu.py runs them on the GPU, together with check_forward_and_files
(MetricComputer.forward and compute_metrics), which pushes images through the LPIPS network at 256^2, as the reference does, and is
therefore nothing the emulator can run in seconds: it has no CPU run.

SSIM.  The yardstick is an fp64 restatement of what skimage.metrics.structural_similarity(win_size=11, gaussian_weights=True,
data_range=1.0, channel_axis=0) computes, written with scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5, mode="reflect"), C1 and
C2 as in skimage, a crop of 5 and the mean (skimage itself is not installed where the suite runs).  cov_norm = 1 is the published
definition (skimage's use_sample_covariance=False), which compute_ssim is held to, within the bar tests/ssim_util.py uses for the
kernel (max(4 x the error of the fp32 restatement, 2e-6)).  skimage's default use_sample_covariance=True, which the reference's call
leaves on, is cov_norm = 121 / 120; how far that moves the value is printed and bounded loosely (dgs_amd/metrics.py says why it is not
reproduced)."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

import lpips_util as LU
import ssim_util as SU
from dgs_amd import metrics
from dgs_amd.lpips import LPIPS

SSIM_SIZES = [(11, 11), (16, 23), (64, 64)]      # one window; odd sizes; several tiles' worth of windows


def skimage_ssim(x, y, cov_norm=1.0):
    """x, y [C, H, W] -> the mean structural similarity as skimage defines it, in fp64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
    gf = lambda a: gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")
    per_channel = []
    for a, b in zip(x, y):
        ux, uy = gf(a), gf(b)
        vx, vy, vxy = cov_norm * (gf(a * a) - ux * ux), cov_norm * (gf(b * b) - uy * uy), cov_norm * (gf(a * b) - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        per_channel.append(S[5:-5, 5:-5].mean())
    return float(np.mean(per_channel))


def _computer(device, with_weights=False):
    if with_weights:
        return metrics.MetricComputer(LU.model(device), lib=LU.lib_of(device) if device == "cpu" else None)
    return metrics.MetricComputer(LPIPS(net="vgg"), lib=LU.lib_of(device) if device == "cpu" else None)


def check_ssim(device, h, w):
    mc = _computer(device)
    pairs = [SU.noise_pair((2, 3, h, w), seed=h * 100 + w)]
    if h == w:
        pairs.append(SU.render_like_pair(2, 3, h, seed=h))
    for x, y in pairs:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
        got = mc.compute_ssim(y.to(device), x.to(device)).cpu().double()
        assert tuple(got.shape) == (2,)
        want = torch.tensor([skimage_ssim(y[i], x[i]) for i in range(2)], dtype=torch.float64)
        bound, e32 = SU.value_bound(SU.ssim_ref(x.double(), y.double()), SU.ssim_ref(x, y))
        err = float((got - want).abs().max())
        sample = torch.tensor([skimage_ssim(y[i], x[i], cov_norm=121.0 / 120.0) for i in range(2)], dtype=torch.float64)
        print(f"ssim {h}x{w}: |compute_ssim - skimage definition (fp64)| = {err:.3e}, bar {bound:.3e} (fp32 restatement {e32:.3e}); "
              f"use_sample_covariance=True would move the value by {float((sample - want).abs().max()):.3e}")
        assert err <= bound, (err, bound)
        assert float((sample - want).abs().max()) < 5e-3


def check_psnr(device):
    mc = _computer(device)
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(3, 3, 20, 27, generator=g) * 1.6 - 0.3            # values below 0 and above 1: the clamp matters
    pred = gt + 0.2 * torch.randn(3, 3, 20, 27, generator=g)
    assert bool((gt < 0).any()) and bool((gt > 1).any()) and bool((pred < 0).any()) and bool((pred > 1).any())
    want = -10 * torch.log10(((gt.double().clamp(0, 1) - pred.double().clamp(0, 1)) ** 2).mean(dim=(1, 2, 3)))
    unclamped = -10 * torch.log10(((gt.double() - pred.double()) ** 2).mean(dim=(1, 2, 3)))
    got = mc.compute_psnr(gt.to(device), pred.to(device)).cpu().double()
    assert tuple(got.shape) == (3,)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-5), (got, want)
    assert float((want - unclamped).abs().min()) > 0.1


def check_forward_and_files(device, directory):
    """MetricComputer.forward on [b, v, 3, h, w] and compute_metrics on three files; LPIPS runs at 256^2."""
    mc = _computer(device, with_weights=True)
    g = torch.Generator().manual_seed(21)
    files = []
    for i in range(3):
        image = torch.rand(2, 3, 24, 32, generator=g)
        files.append({"render_images": (image + 0.05 * torch.randn(2, 3, 24, 32, generator=g)), "image": image})
        torch.save(files[-1], os.path.join(directory, f"scene_{i}.pt"))
    with open(os.path.join(directory, "notes.txt"), "w") as f:      # not a .pt file: skipped
        f.write("x")
    renders = torch.stack([f["render_images"] for f in files]).to(device)          # [3, 2, 3, 24, 32]
    images = torch.stack([f["image"] for f in files]).to(device)
    psnr, ssim, lp = mc(renders, images)
    assert all(tuple(t.shape) == (6,) and t.device == renders.device and t.dtype == torch.float32 for t in (psnr, ssim, lp))
    # forward is the three per-image calls on the flattened batch
    flat_r, flat_i = renders.flatten(0, 1), images.flatten(0, 1)
    assert LU.same_bytes(psnr, mc.compute_psnr(flat_r, flat_i)) and LU.same_bytes(ssim, mc.compute_ssim(flat_r, flat_i))
    assert LU.same_bytes(lp, mc.compute_lpips(flat_r, flat_i))
    # compute_lpips is the 256^2 resize to (-1, 1), then the network
    up = lambda t: torch.nn.functional.interpolate(t, size=[256, 256], mode="bilinear") * 2.0 - 1.0
    direct = mc.lpips_loss_module(up(flat_i), up(flat_r)).reshape(-1)
    assert torch.allclose(lp, direct, rtol=1e-4, atol=1e-7), (lp, direct)
    assert bool((lp > 0).all()) and bool((ssim < 1).all()) and bool((psnr > 10).all())
    # compute_metrics: chunks of 2 files (a full chunk and a rest), the reference's JSON
    result = metrics.compute_metrics(directory, chunk=2, lpips=mc.lpips_loss_module)
    with open(os.path.join(directory, "eval_result.json")) as f:
        written = json.load(f)
    assert list(written) == ["psnr", "ssim", "lpips"] and tuple(written.values()) == result
    for got, per_image in zip(result, (psnr, ssim, lp)):
        assert got == per_image.mean().item(), (got, per_image.mean().item())


@pytest.mark.parametrize("size", SSIM_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_compute_ssim_is_the_skimage_definition(size):
    check_ssim("cpu", *size)


def test_compute_psnr_clamps():
    check_psnr("cpu")


def test_surface(tmp_path):
    with pytest.raises(TypeError):
        metrics.MetricComputer(torch.nn.Identity())
    with pytest.raises(ValueError, match="weights"):
        metrics.compute_metrics(str(tmp_path), lpips=None)
    with pytest.raises(ValueError, match="no .pt file"):
        metrics.compute_metrics(str(tmp_path), lpips=LPIPS(net="vgg"))
    mc = _computer("cpu")
    with pytest.raises(RuntimeError, match="no weights"):          # PSNR and SSIM need no weights; LPIPS says that it has none
        mc.compute_lpips(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))
