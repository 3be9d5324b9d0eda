"""Loss consumers on the device: per-sample MSE + PSNR and the MSE gradient in one pass, the SSIM
term fused with them, the LPIPS input resize, and the two terms on the denoiser's pixel-aligned points (points-distribution and xyz
loss) with their gradient, and the reference's weight schedules (`scheduled_weight`).

Mirrors diffusionGS/utils/losses.py: the `l2_loss` / `psnr` terms of LossComputer.forward (:281-285, :303), `compute_psnr`
(:399-402), `SsimLoss` (:216-234, :317-321), `l2_loss_xyz` (:288-292) and `pointsdist_loss` (:325-364).  The LPIPS network is
dgs_amd.lpips (the metric, and with differentiable=True the loss term with its input gradient); MetricComputer (:373-473), its compute_ssim included, is
dgs_amd.metrics, which says how skimage's operator relates to `ssim` here.
csrc/loss.hip and csrc/ssim.hip through include/dgs_loss.h; no CPU fallback."""
import ctypes

import torch

from . import _native


def _run(rendering, target, clamp01, want_psnr, grad_scale, lib):
    assert rendering.shape == target.shape and rendering.dtype == torch.float32 and target.dtype == torch.float32
    r, t = rendering.contiguous(), target.contiguous()
    B = r.shape[0]
    n = r[0].numel()
    dev = r.device
    l2 = torch.empty(B, dtype=torch.float32, device=dev)
    psnr = torch.empty(B, dtype=torch.float32, device=dev) if want_psnr else None
    grad = torch.empty_like(r) if grad_scale is not None else None
    partial = torch.empty(B, _native.LOSS_CHUNKS, dtype=torch.float32, device=dev)
    a = _native.DgsMseArgs()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    a.B, a.n, a.rendering, a.target, a.clamp01 = B, n, ptr(r), ptr(t), int(clamp01)
    a.l2, a.psnr, a.grad, a.grad_scale, a.partial = ptr(l2), ptr(psnr), ptr(grad), float(grad_scale or 0.0), ptr(partial)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if r.is_cuda else None
    rc = (lib or _native.lib()).dgs_mse_psnr(ctypes.byref(a), stream)
    if rc != 0:
        raise RuntimeError(f"dgs_mse_psnr failed: {rc}")
    return l2, psnr, grad


def compute_psnr(ground_truth, predicted, lib=None):
    """losses.py:399-402: clamp to [0, 1], per-image mean squared error over (c, h, w), -10 log10."""
    return _run(predicted, ground_truth, True, True, None, lib)[1]


class _Mse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendering, target, lib):
        B = rendering.shape[0]
        l2, psnr, grad = _run(rendering, target, False, True, 1.0 / B, lib)     # d(mean_b l2_b) / d rendering
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(psnr)
        return l2.mean(), l2, psnr

    @staticmethod
    def backward(ctx, g_loss, g_l2, _g_psnr):
        (grad,) = ctx.saved_tensors
        out = grad * g_loss
        if g_l2 is not None:     # per-sample weights: d l2_b / d rendering = B * grad_b
            out = out + grad * (g_l2 * grad.shape[0]).reshape(-1, *([1] * (grad.dim() - 1)))
        return out, None, None


def mse_psnr(rendering, target, lib=None):
    """rendering / target [b, v, 3, h, w] -> (loss = mean_b l2_b, l2 [b], psnr [b]); loss and l2 are differentiable w.r.t.
    `rendering` (the gradient was produced by the same pass that formed the sums)."""
    return _Mse.apply(rendering, target, lib)


def _resize_args(x_shape, size, lib):
    a = _native.DgsResizeArgs()
    a.planes = 1
    for d in x_shape[:-2]:
        a.planes *= int(d)
    a.in_h, a.in_w, a.out_h, a.out_w = int(x_shape[-2]), int(x_shape[-1]), int(size[0]), int(size[1])
    return a, (lib or _native.lib())


class _LpipsInput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, mul, add, lib):
        x = x.contiguous().float()
        out = torch.empty(tuple(x.shape[:-2]) + tuple(size), dtype=torch.float32, device=x.device)
        a, L = _resize_args(x.shape, size, lib)
        a.src, a.dst, a.mul, a.add = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), float(mul), float(add)
        stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream) if x.is_cuda else None
        rc = L.dgs_resize_bilinear(ctypes.byref(a), stream)
        if rc != 0:
            raise RuntimeError(f"dgs_resize_bilinear failed: {rc}")
        ctx.meta = (tuple(x.shape), tuple(size), float(mul), lib)
        return out

    @staticmethod
    def backward(ctx, g):
        shape, size, mul, lib = ctx.meta
        g = g.contiguous().float()
        dx = torch.empty(shape, dtype=torch.float32, device=g.device)
        a, L = _resize_args(shape, size, lib)
        a.ddst, a.dsrc, a.mul = ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(dx.data_ptr()), mul
        stream = ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream) if g.is_cuda else None
        rc = L.dgs_resize_bilinear_backward(ctypes.byref(a), stream)
        if rc != 0:
            raise RuntimeError(f"dgs_resize_bilinear_backward failed: {rc}")
        return dx, None, None, None, None


def lpips_input(images, size=(256, 256), lib=None):
    """losses.py:304-309: `F.interpolate(images, size=[256, 256], mode='bilinear') * 2.0 - 1.0` -- what the reference feeds its
    LPIPS module for renderings and targets ([n, 3, h, w] in (0, 1) -> [n, 3, 256, 256] in (-1, 1)), one fused launch,
    differentiable.  The network behind it is dgs_amd.lpips.LPIPS (differentiable=True for a loss term)."""
    return _LpipsInput.apply(images, tuple(size), 2.0, -1.0, lib)


def _points_call(aligned, ray_o, gt, masks, w_pd, w_xyz, want_grad, lib, denominator=None, w_xyz_dev=None):
    B, V, C, H, W = aligned.shape
    assert C == 3 and ray_o.shape == aligned.shape
    dev = aligned.device
    L = lib or _native.lib()
    f = lambda x: None if x is None else x.contiguous().float()
    al, ro, gt, masks = f(aligned), f(ray_o), f(gt), f(masks)
    if gt is not None:
        assert masks is not None and tuple(masks.shape) == (B, V, 1, H, W) and gt.shape == aligned.shape
    pd = torch.empty(B, dtype=torch.float32, device=dev)
    xyz = torch.zeros(1, dtype=torch.float32, device=dev)
    grad = torch.empty_like(al) if want_grad else None
    ws = torch.empty(int(L.dgs_points_loss_workspace_floats(B, V)), dtype=torch.float32, device=dev)
    wpd = f(w_pd)
    a = _native.DgsPointsLossArgs()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    a.B, a.V, a.H, a.W = B, V, H, W
    a.aligned, a.ray_o, a.gt, a.masks, a.pointsdist, a.xyz = ptr(al), ptr(ro), ptr(gt), ptr(masks), ptr(pd), ptr(xyz)
    a.w_pointsdist, a.w_xyz, a.grad, a.workspace = ptr(wpd), float(w_xyz), ptr(grad), ptr(ws)
    if denominator is not None or w_xyz_dev is not None:
        if not hasattr(L, "dgs_train_inputs"):         # the two fields came with that symbol: an older build would silently ignore them
            raise RuntimeError("dgs_amd: this library build predates DgsPointsLossArgs.xyz_denominator -- rebuild it (`python -m dgs_amd.build`)")
        denominator, w_xyz_dev = f(denominator), f(w_xyz_dev)
        a.xyz_denominator, a.w_xyz_dev = ptr(denominator), ptr(w_xyz_dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if al.is_cuda else None
    rc = L.dgs_points_loss(ctypes.byref(a), stream)
    if rc != 0:
        raise RuntimeError(f"dgs_points_loss failed: {rc}")
    return pd, xyz[0], grad


class _PointsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, aligned, ray_o, gt, masks, lib):
        pd, xyz, _ = _points_call(aligned, ray_o, gt, masks, None, 0.0, False, lib)
        ctx.save_for_backward(aligned, ray_o, *([gt, masks] if gt is not None else []))
        ctx.lib = lib
        return pd, xyz

    @staticmethod
    def backward(ctx, g_pd, g_xyz):
        aligned, ray_o, *rest = ctx.saved_tensors
        gt, masks = rest if rest else (None, None)
        w_pd = g_pd if g_pd is not None else torch.zeros(aligned.shape[0], device=aligned.device)
        w_xyz = float(g_xyz) if (g_xyz is not None and gt is not None) else 0.0      # one host read of a scalar; 0 without a gt
        _, _, grad = _points_call(aligned, ray_o, gt, masks, w_pd, w_xyz, True, ctx.lib)
        return grad.to(aligned.dtype), None, None, None, None


def points_losses(img_aligned_xyz, ray_o, gt_img_aligned_xyz=None, masks=None, lib=None):
    """losses.py:288-292,325-364 on the device: -> (pointsdist_loss [b], l2_loss_xyz scalar -- 0 without a gt), both differentiable
    w.r.t. `img_aligned_xyz` [b, v, 3, h, w] (the statistics of the points-distribution target are detached, as in the reference).
    `masks` [b, v, 1, h, w] is the reference's `masks_input`."""
    return _PointsLoss.apply(img_aligned_xyz, ray_o, gt_img_aligned_xyz, masks, lib)


class _PointsLossPart(torch.autograd.Function):
    """points_losses of a micro-batch whose xyz term is divided by a mask sum given on the device; the upstream gradient of xyz stays
    on the device as well (DgsPointsLossArgs.xyz_denominator / w_xyz_dev): no host read in either direction."""

    @staticmethod
    def forward(ctx, aligned, ray_o, gt, masks, denominator, lib):
        pd, xyz, _ = _points_call(aligned, ray_o, gt, masks, None, 0.0, False, lib, denominator=denominator)
        ctx.save_for_backward(aligned, ray_o, gt, masks, denominator)
        ctx.lib = lib
        return pd, xyz

    @staticmethod
    def backward(ctx, g_pd, g_xyz):
        aligned, ray_o, gt, masks, denominator = ctx.saved_tensors
        dev = aligned.device
        w_pd = g_pd if g_pd is not None else torch.zeros(aligned.shape[0], device=dev)
        w_dev = g_xyz.reshape(1) if g_xyz is not None else torch.zeros(1, device=dev)
        _, _, grad = _points_call(aligned, ray_o, gt, masks, w_pd, 1.0, True, ctx.lib, denominator=denominator, w_xyz_dev=w_dev)
        return grad.to(aligned.dtype), None, None, None, None, None


def points_losses_part(img_aligned_xyz, ray_o, gt_img_aligned_xyz, masks, mask_sum, lib=None):
    """`points_losses` for a PART of a batch: -> (pointsdist_loss [b] of the part, sum((aligned m - gt m)^2) of the part / mask_sum).
    `mask_sum` is a device float tensor of one element, the whole batch's `masks.sum()`: the parts' xyz terms then add up to the
    reference's scalar (losses.py:288-292) and their gradients to its gradient.  Nothing is read back to the host."""
    return _PointsLossPart.apply(img_aligned_xyz, ray_o, gt_img_aligned_xyz, masks, mask_sum.reshape(1), lib)


def scheduled_weight(value, global_step, epoch=0):
    """`C()` of the reference (utils/misc.py:73-94), which turns an entry of `system.loss` into the weight of this step: a number is
    returned as it is; a list [start_step, start_value, end_value, end_step] (three values: start_step = 0) interpolates linearly
    between the two values and clamps outside -- over optimizer steps when end_step is an int, over epochs when it is a float.
    `lambda_pointsdist: [150, 1., 0., 151]` of configs/diffusionGS_rel.yaml is 1 up to step 150 and 0 from step 151."""
    if isinstance(value, (int, float)):
        return value
    if isinstance(value, tuple) or type(value).__name__ == "ListConfig":      # config_to_primitive: an OmegaConf list is a list
        value = list(value)
    if not isinstance(value, list):
        raise TypeError("Scalar specification only supports list, got", type(value))
    if len(value) == 3:
        value = [0] + value
    if len(value) != 4:
        raise ValueError(f"a schedule has 3 or 4 entries, got {len(value)}")
    start_step, start_value, end_value, end_step = value
    if isinstance(end_step, int):
        current = global_step
    elif isinstance(end_step, float):
        current = epoch
    else:
        raise TypeError("Scalar specification: end_step is an int (steps) or a float (epochs), got", type(end_step))
    return start_value + (end_value - start_value) * max(min(1.0, (current - start_step) / (end_step - start_step)), 0.0)


SSIM_WINDOW = 11


def _ssim_views(x, y):
    """[N, C, H, W] or [b, v, C, H, W] -> contiguous f32 [N, C, H, W] pair and the number of samples b (N for 4-d input)."""
    if x.shape != y.shape or x.dim() not in (4, 5):
        raise ValueError(f"ssim: expected two [N, C, H, W] or [b, v, C, H, W] tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("ssim: float32 tensors expected")
    if x.shape[-2] < SSIM_WINDOW or x.shape[-1] < SSIM_WINDOW:
        raise ValueError(f"ssim: planes of {x.shape[-2]} x {x.shape[-1]} are smaller than the {SSIM_WINDOW}-tap window")
    samples = x.shape[0]
    return x.reshape(-1, *x.shape[-3:]).contiguous(), y.reshape(-1, *y.shape[-3:]).contiguous(), samples


def _ssim_args(x, y, samples, data_range, saved):
    a = _native.DgsSsimArgs()
    a.N, a.C, a.H, a.W = (int(d) for d in x.shape)
    a.B, a.data_range = int(samples), float(data_range)
    a.x, a.y, a.saved = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(saved.data_ptr()) if saved is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream) if x.is_cuda else None
    return a, stream


def _ssim_forward(x, y, samples, data_range, want_mse, want_saved, lib):
    L = lib or _native.lib()
    N, C, H, W = x.shape
    dev = x.device
    new = lambda n: torch.empty(int(n), dtype=torch.float32, device=dev)
    saved = new(L.dgs_ssim_saved_floats(N, C, H, W)) if want_saved else None
    out, ws = new(N), new(L.dgs_ssim_workspace_floats(N, C, H, W))
    l2, psnr = (new(samples), new(samples)) if want_mse else (None, None)
    a, stream = _ssim_args(x, y, samples, data_range, saved)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    a.ssim, a.l2, a.psnr, a.workspace = ptr(out), ptr(l2), ptr(psnr), ptr(ws)
    rc = L.dgs_ssim(ctypes.byref(a), stream)
    if rc != 0:
        raise RuntimeError(f"dgs_ssim failed: {rc}")
    return out, l2, psnr, saved


def _ssim_backward(x, y, samples, data_range, saved, g, mse_scale, lib):
    L = lib or _native.lib()
    dx = torch.empty_like(x)
    g = g.contiguous().float()                                       # no copies when they already are f32 and dense
    mse_scale = mse_scale.contiguous().float() if mse_scale is not None else None
    a, stream = _ssim_args(x, y, samples, data_range, saved)
    a.g, a.dx = ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(dx.data_ptr())
    a.mse_scale = ctypes.c_void_p(mse_scale.data_ptr()) if mse_scale is not None else None
    rc = L.dgs_ssim_backward(ctypes.byref(a), stream)
    if rc != 0:
        raise RuntimeError(f"dgs_ssim_backward failed: {rc}")
    return dx


class _Ssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, data_range, lib):
        xs, ys, _ = _ssim_views(x, y)
        need = ctx.needs_input_grad[0]
        out, _, _, saved = _ssim_forward(xs, ys, xs.shape[0], data_range, False, need, lib)
        if need:
            ctx.save_for_backward(xs, ys, saved)
        ctx.meta = (tuple(x.shape), data_range, lib)
        return out

    @staticmethod
    def backward(ctx, g):
        xs, ys, saved = ctx.saved_tensors
        shape, data_range, lib = ctx.meta
        return _ssim_backward(xs, ys, xs.shape[0], data_range, saved, g, None, lib).reshape(shape), None, None, None


def ssim(x, y, data_range=1.0, lib=None):
    """pytorch_msssim.SSIM(win_size=11, win_sigma=1.5, data_range, size_average=False) of `x` against `y` ([N, C, H, W] or
    [b, v, C, H, W], float32) -> [N] (N = b * v), differentiable in `x`.  One fused launch each way (csrc/ssim.hip)."""
    return _Ssim.apply(x, y, float(data_range), lib)


def ssim_loss(rendering, target, lib=None):
    """losses.py:317-321: `(1 - ssim).reshape(b, v).mean(dim=1)` for rendering / target [b, v, 3, h, w] -> [b]."""
    if rendering.dim() != 5:
        raise ValueError("ssim_loss: [b, v, C, h, w] tensors expected")
    b, v = rendering.shape[:2]
    return (1.0 - ssim(rendering, target, 1.0, lib)).reshape(b, v).mean(dim=1)


_coef_cache = {}


def _coefs(key, values, dev):
    """A small constant vector on the device, built once per (shape, weights, device)."""
    k = (key, values, str(dev))
    if k not in _coef_cache:
        _coef_cache[k] = torch.tensor(values, dtype=torch.float32, device=dev)
    return _coef_cache[k]


class _ImageLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendering, target, lambda_mse, lambda_ssim, lib):
        xs, ys, b = _ssim_views(rendering, target)
        v = xs.shape[0] // b
        need = ctx.needs_input_grad[0]
        s, l2, psnr, saved = _ssim_forward(xs, ys, b, 1.0, True, need, lib)
        sl = (1.0 - s).reshape(b, v).mean(dim=1)                     # the reference's expression (ssim_loss above)
        # lambda_mse * l2.mean() + lambda_ssim * sl.mean() as one dot product with a constant vector
        loss = torch.dot(torch.cat([l2, sl]), _coefs("fwd", (lambda_mse / b,) * b + (lambda_ssim / b,) * b, xs.device))
        if need:
            ctx.save_for_backward(xs, ys, saved)
        ctx.meta = (tuple(rendering.shape), b, v, lambda_mse, lambda_ssim, lib)
        ctx.mark_non_differentiable(psnr)
        ctx.set_materialize_grads(False)
        return loss, l2, psnr, sl

    @staticmethod
    def backward(ctx, g_loss, g_l2, _g_psnr, g_sl):
        xs, ys, saved = ctx.saved_tensors
        shape, b, v, lambda_mse, lambda_ssim, lib = ctx.meta
        dev = xs.device
        # d / d l2[b] and d / d ssim[n] of whatever was built on the outputs, folded into the one backward launch: [b] weights of the
        # squared-error sums followed by [N] weights of the images' ssim (d ssim_loss[b] / d ssim[n] = -1 / v)
        n = b * v
        if g_loss is not None:
            w = g_loss.reshape(1) * _coefs("bwd", (lambda_mse / b,) * b + (-lambda_ssim / n,) * n, dev)
        else:
            w = torch.zeros(b + n, dtype=torch.float32, device=dev)
        if g_l2 is not None:
            w[:b] += g_l2
        if g_sl is not None:
            w[b:] -= (g_sl * (1.0 / v)).repeat_interleave(v)
        return _ssim_backward(xs, ys, b, 1.0, saved, w[b:], w[:b], lib).reshape(shape), None, None, None, None


def image_losses(rendering, target, lambda_mse=1.0, lambda_ssim=0.0, lib=None):
    """rendering / target [b, v, C, h, w] -> (loss, l2 [b], psnr [b], ssim_loss [b]) with
    loss = lambda_mse * l2.mean() + lambda_ssim * ssim_loss.mean() (how PointDiffusionSystem combines the two image terms,
    systems/diffusion_gs_system.py:94-128).  One autograd node: the forward is dgs_ssim (the squared-error sums ride along), the
    backward ONE dgs_ssim_backward launch that writes d loss / d rendering of both terms in a single store.  loss, l2 and
    ssim_loss are differentiable w.r.t. `rendering`."""
    if rendering.dim() != 5:
        raise ValueError("image_losses: [b, v, C, h, w] tensors expected")
    return _ImageLosses.apply(rendering, target, float(lambda_mse), float(lambda_ssim), lib)
