"""Yardstick of the SSIM tests: a restatement in torch of the published formula that `pytorch_msssim.SSIM(win_size=11,
win_sigma=1.5, data_range, size_average=False)` implements (include/dgs_loss.h DgsSsimArgs states it).  The tests are pinned to THIS
FORMULA, not to the library's binary: pytorch_msssim is not installed where the suite runs, so no fixture could be minted from it.

Values come from the fp64 evaluation, gradients from autograd of it.  The same code evaluated in plain fp32 gives `e32`, what a
straightforward fp32 implementation of the formula loses (the cancellation in G(x x) - mu1^2 against C2 = 9e-4 on flat regions
dominates); the product must stay within max(4 * e32, floor): 4 because the kernel sums the 121 taps and the tile means in another
order than conv2d, the floors from what the suite already demands of a loss value (2e-6, tests/test_losses.py) and of a gradient
(2e-4 of the tensor's max).  Reads nothing outside the repository."""
import torch
import torch.nn.functional as F

VALUE_FLOOR = 2e-6
GRAD_FLOOR = 2e-4


def window(dtype):
    k = torch.arange(11, dtype=torch.float32) - 5.0
    w = torch.exp(-(k ** 2) / (2 * 1.5 ** 2))
    return (w / w.sum()).to(dtype)                       # built in fp32, cast to the working dtype


def _filter(img, w):
    C = img.shape[1]
    img = F.conv2d(img, w.reshape(1, 1, 11, 1).repeat(C, 1, 1, 1), groups=C)       # along H
    return F.conv2d(img, w.reshape(1, 1, 1, 11).repeat(C, 1, 1, 1), groups=C)      # along W, VALID


def ssim_ref(x, y, data_range=1.0):
    """x, y [N, C, H, W] of one dtype -> ssim [N] (size_average=False)."""
    w = window(x.dtype).to(x.device)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = _filter(x, w), _filter(y, w)
    s1 = _filter(x * x, w) - mu1 * mu1
    s2 = _filter(y * y, w) - mu2 * mu2
    s12 = _filter(x * y, w) - mu1 * mu2
    m = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * ((2 * s12 + C2) / (s1 + s2 + C2))
    return m.flatten(2).mean(-1).mean(-1)


def image_loss_ref(x, y, lambda_mse, lambda_ssim):
    """x, y [b, v, C, H, W] -> (loss, l2 [b], ssim_loss [b]) as losses.image_losses defines them."""
    b, v = x.shape[:2]
    l2 = ((x - y) ** 2).mean(dim=(1, 2, 3, 4))
    sl = (1.0 - ssim_ref(x.flatten(0, 1), y.flatten(0, 1))).reshape(b, v).mean(dim=1)
    return lambda_mse * l2.mean() + lambda_ssim * sl.mean(), l2, sl


def weighted_grad(fn, x, dtype):
    """d fn(x) / d x for a scalar-valued fn, evaluated in `dtype` on the CPU."""
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    fn(xx).backward()
    return xx.grad


def value_bound(ref64, ref32):
    e32 = float((ref32.detach().double() - ref64.detach()).abs().max())
    return max(4 * e32, VALUE_FLOOR), e32


def grad_bound(g64, g32):
    """-> (allowed max abs deviation, e32 relative to the fp64 gradient's max, that max)."""
    top = float(g64.abs().max())
    e32 = float((g32.double() - g64).abs().max()) / top
    return max(4 * e32, GRAD_FLOOR) * top, e32, top


def noise_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 1.4 - 0.2, torch.rand(shape, generator=g)


def render_like_pair(n, c, res, seed, noise=0.01):
    """Exactly flat white background on both images, a smooth textured blob in the middle, x = y + small noise inside the blob: where
    s1 + s2 is ~0 and C2 alone holds the denominator."""
    g = torch.Generator().manual_seed(seed)
    u = torch.linspace(-1, 1, res)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    ph = torch.rand(n, c, 1, 1, generator=g) * 6.28
    cx, cy = torch.rand(n, 1, 1, 1, generator=g) * 0.4 - 0.2, torch.rand(n, 1, 1, 1, generator=g) * 0.4 - 0.2
    r2 = (xx - cx) ** 2 + (yy - cy) ** 2
    alpha = torch.clamp((0.45 - r2.sqrt()) * 12.0, 0.0, 1.0)                      # 1 inside, 0 outside, a soft rim
    tex = 0.5 + 0.25 * torch.sin(9.0 * xx + ph) * torch.cos(7.0 * yy - ph) + 0.1 * torch.sin(23.0 * (xx + yy) + 2 * ph)
    y = (alpha * tex + (1.0 - alpha)).contiguous()
    x = (y + noise * torch.randn(n, c, res, res, generator=g) * (alpha > 0)).contiguous()
    assert bool((y[..., 0, :] == 1.0).all()) and bool((x[..., 0, :] == 1.0).all())
    return x, y
