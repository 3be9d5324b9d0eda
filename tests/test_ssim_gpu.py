"""Fused SSIM loss on the MI355X (product library) at the shapes that ship, against the fp64 restatement of the published formula
(tests/ssim_util.py; the checks are those of tests/test_ssim.py).  Every case is a plain launch on valid buffers.
DGS_SSIM_PARITY=<file> appends the measured deviations of each case (profiles/ssim_parity.txt comes from it)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ssim_util as U  # noqa: E402
from test_ssim import check_identical_images, check_image_losses, check_ssim_case  # noqa: E402

GPU_CASES = {
    "render_like_40x3x256": (lambda: U.render_like_pair(40, 3, 256, 11), 4),      # b = 4, v = 10 at 256^2
    "render_like_8x3x512": (lambda: U.render_like_pair(8, 3, 512, 12), 2),
    "noise_6x3x256": (lambda: U.noise_pair((6, 3, 256, 256), 13), 3),
    "odd_5x3x131x203": (lambda: U.noise_pair((5, 3, 131, 203), 14), 1),           # the scalar staging path, partial tiles both ways
}


def _report(lines):
    path = os.environ.get("DGS_SSIM_PARITY")
    if path:
        with open(path, "a") as f:
            f.write("".join(ln + "\n" for ln in lines))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_ssim_values_and_gradient_on_gpu(name):
    make, _ = GPU_CASES[name]
    x, y = make()
    lines = []
    check_ssim_case(name, x, y, None, torch.device("cuda:0"), lines)
    _report(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_image_losses_on_gpu(name):
    make, b = GPU_CASES[name]
    x, y = make()
    lines = []
    check_image_losses(name, x, y, b, None, torch.device("cuda:0"), lines)
    _report(lines)


@pytest.mark.gpu
def test_identical_images_on_gpu():
    check_identical_images(None, torch.device("cuda:0"), shape=(4, 3, 256, 256))


@pytest.mark.gpu
def test_trainer_step_with_the_ssim_term_on_gpu():
    """One DataParallelTrainer step with lambda_ssim=0.2 at the model of tests/test_optim.py's GPU trainer tests (width 1024, two
    layers, 64^2 views): finite, different from the MSE-only step, and two runs from the same state agree bit for bit."""
    import numpy as np
    from dgs_amd import cameras, synth
    from dgs_amd import denoiser as dn
    from dgs_amd.optim import FusedAdamW
    from dgs_amd.train import DataParallelTrainer
    dev = torch.device("cuda:0")
    batch, t = synth.make_batch(1, 64, V=4, device=dev, seed=5, with_t=True)
    rc2w = torch.tensor(np.stack([cameras.ring_cameras(2, phase_deg=5.0)])).to(dev)
    rk = torch.tensor(cameras.default_fxfycxcy(64)).expand(1, 2, 4).contiguous().to(dev)
    target = torch.rand(1, 2, 3, 64, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def run(lambda_ssim):
        m = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=2), device=dev)
        m.reset_parameters(seed=2)
        m = m.to(dev)
        m.train()
        with DataParallelTrainer(m, FusedAdamW(m, lr=1e-3), lambda_ssim=lambda_ssim) as tr:
            loss = float(tr.step(batch, t, target, rc2w, rk))
            term = None if tr.last_ssim_loss is None else tr.last_ssim_loss.clone()
        return loss, term, {n: p.detach().clone() for n, p in m.named_parameters()}

    loss_a, term_a, pa = run(0.2)
    loss_b, term_b, pb = run(0.2)
    loss_m, term_m, pm = run(None)
    assert term_m is None and term_a.shape == (1,) and bool(torch.isfinite(term_a).all())
    assert np.isfinite(loss_a) and all(bool(torch.isfinite(p).all()) for p in pa.values())
    assert loss_a == loss_b and torch.equal(term_a, term_b)
    assert not [n for n in pa if not torch.equal(pa[n], pb[n])]
    assert loss_a > loss_m and any(not torch.equal(pa[n], pm[n]) for n in pa)
    assert abs(loss_a - (loss_m + 0.2 * float(term_a.mean()))) <= 1e-5 * abs(loss_a)
