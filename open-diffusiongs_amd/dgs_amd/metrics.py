"""The reference's evaluation on the device: `MetricComputer` (diffusionGS/utils/losses.py:373-473) and `compute_metrics`
(eval_scene_result.py) -- PSNR, SSIM and LPIPS per image, from HIP kernels, with no `lpips`, `skimage` or `torchvision` behind them.

    compute_psnr    clamp to [0, 1], per-image mean squared error, -10 log10: dgs_mse_psnr (csrc/loss.hip)
    compute_ssim    csrc/ssim.hip through losses.ssim (below)
    compute_lpips   the 256^2 resize of losses.lpips_input, then dgs_amd.lpips.LPIPS (csrc/lpips.hip)

SSIM.  The reference calls `skimage.metrics.structural_similarity(gt, pred, win_size=11, gaussian_weights=True, channel_axis=0,
data_range=1.0)` in a host loop.  With gaussian_weights that is a Gaussian filter of sigma 1.5 truncated at 3.5 sigma (radius 5, the
same 11 normalised taps as ssim.hip) over the reflect-padded image, the SSIM map, a crop of 5 pixels at every border and the mean.
The crop removes exactly the pixels whose window touched the padding, so the filter part is the VALID-window filter that ssim.hip
computes, with the same C1 = 0.01^2, C2 = 0.03^2; tests/test_metrics.py checks that against an fp64 restatement built on
scipy.ndimage.gaussian_filter.  One difference remains and is NOT reproduced: the reference leaves skimage's `use_sample_covariance`
at its default True, which multiplies the two variances and the covariance by 121 / 120 before they enter the formula
(skimage's documentation names use_sample_covariance=False as the setting that matches Wang et al.).  compute_ssim returns the
published (Wang et al., pytorch_msssim) value; the reference's number differs from it by that factor's effect, up to 4e-5 on the
suite's image pairs (tests/test_metrics.py prints it).  This is written from memory of skimage, which is not installed where the
library is built.

All three return f32 [n] tensors on the inputs' device; nothing is read back before `compute_metrics` forms its means."""
import json
import os

import torch
import torch.nn as nn

from . import losses
from .lpips import LPIPS


class MetricComputer(nn.Module):
    """`MetricComputer(lpips)`: `lpips` is a dgs_amd.lpips.LPIPS with its weights loaded (the library ships none)."""

    def __init__(self, lpips, lib=None):
        super().__init__()
        if not isinstance(lpips, LPIPS):
            raise TypeError("MetricComputer: a dgs_amd.lpips.LPIPS module expected")
        self.lpips_loss_module = lpips.eval()
        self._lib = lib

    @torch.no_grad()
    def compute_psnr(self, ground_truth, predicted):
        """[n, c, h, w] x 2 -> [n]."""
        return losses.compute_psnr(ground_truth.float(), predicted.float(), lib=self._lib)

    @torch.no_grad()
    def compute_ssim(self, ground_truth, predicted):
        """[n, c, h, w] x 2, h, w >= 11 -> [n] (see the module's docstring for what it is and is not)."""
        return losses.ssim(predicted.float(), ground_truth.float(), 1.0, self._lib)

    @torch.no_grad()
    def compute_lpips(self, ground_truth, predicted):
        """[n, 3, h, w] x 2 in (0, 1) -> [n]."""
        p = losses.lpips_input(predicted, (256, 256), self._lib)
        g = losses.lpips_input(ground_truth, (256, 256), self._lib)
        return self.lpips_loss_module(p, g).reshape(-1)

    def forward(self, target, rendering):
        """[..., 3, h, w] x 2 -> (psnr, ssim, lpips), each [n] over the flattened leading dimensions."""
        rendering = rendering.reshape(-1, *rendering.shape[-3:])
        target = target.reshape(-1, *target.shape[-3:])
        return self.compute_psnr(target, rendering), self.compute_ssim(target, rendering), self.compute_lpips(target, rendering)


def compute_metrics(path, chunk=8, lpips=None, device=None, lib=None):
    """eval_scene_result.py: every `*.pt` under `path` holds `render_images` and `image` ([v, 3, h, w] each); the metrics are computed
    over chunks of `chunk` files, their means over all images are written to `path`/eval_result.json (keys psnr, ssim, lpips) and
    returned.  Like the reference, MetricComputer is called as (stacked renders, stacked images)."""
    if lpips is None:
        raise ValueError("compute_metrics: pass lpips=<dgs_amd.lpips.LPIPS with weights loaded>; the library ships no weights")
    device = torch.device(device) if device is not None else lpips.scaling_layer.shift.device
    computer = MetricComputer(lpips, lib=lib)
    renders, gts = [], []
    for name in sorted(os.listdir(path)):
        if name.endswith(".pt"):
            pkg = torch.load(os.path.join(path, name), map_location="cpu")
            renders.append(pkg["render_images"])
            gts.append(pkg["image"])
    if not renders:
        raise ValueError(f"compute_metrics: no .pt file under {path}")
    renders, gts = torch.stack(renders), torch.stack(gts)
    psnr, ssim, lp = [], [], []
    for i in range(0, len(renders), chunk):
        a, b, c = computer(renders[i:i + chunk].to(device), gts[i:i + chunk].to(device))
        psnr.append(a)
        ssim.append(b)
        lp.append(c)
    result = {"psnr": torch.cat(psnr).mean().item(), "ssim": torch.cat(ssim).mean().item(), "lpips": torch.cat(lp).mean().item()}
    with open(os.path.join(path, "eval_result.json"), "w") as f:
        json.dump(result, f, indent=4)
    return result["psnr"], result["ssim"], result["lpips"]
