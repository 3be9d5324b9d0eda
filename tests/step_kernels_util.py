"""The kernels that run beside the network in every training and sampling step -- csrc/loss.hip (points-distribution / xyz loss, MSE /
PSNR, the LPIPS input resize), csrc/optim.hip (sum of squares, AdamW + copies) and csrc/sampler.hip -- each against a plain fp64
restatement (or, where the kernel claims the reference's operation order, the fp32 torch expression bit for bit) at the sizes where
their index arithmetic changes: empty chunks, sizes that do not divide, scalar tails, a tile's end, the second trip of a grid-stride loop.

Case tables, references and one check_* per kernel taking (lib, device): tests/test_step_kernels_emu.py runs them on the CPU emulator
build, tests/test_step_kernels_gpu.py on the GPU, tools/step_kernels_error.py prints what they measured (RECORDS).

Every C-level launch writes between guard bands: outputs and workspaces sit inside buffers pre-filled with 7.0, GUARD elements on either
side (and in the padding between the slices of a flat buffer), and the bands must still hold 7.0 afterwards."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from dgs_amd import _native

GUARD = 64              # elements on either side: 256 bytes of fp32, so the guarded view keeps the 16-byte alignment the kernels ask for
FILL = 7.0
RECORDS = []            # (section, case, quantity, kernel error, yardstick error or None, bar, error / bar)


def record(section, case, name, err, yard, bar):
    RECORDS.append((section, case, name, float(err), None if yard is None else float(yard), float(bar), float(err) / float(bar) if bar else 0.0))


def _lib(lib):
    return lib or _native.lib()


def _stream(dev):
    dev = torch.device(dev)
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None


def _ptr(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


class Guarded:
    """`n` elements between two bands of GUARD elements holding 7.0; the payload starts as 7.0 too unless `init` is given."""

    def __init__(self, n, device, dtype=torch.float32, init=None):
        self.whole = torch.full((n + 2 * GUARD,), FILL, dtype=dtype, device=device)
        self.n = n
        self.t = self.whole[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def intact(self):
        return bool((self.whole[:GUARD] == FILL).all()) and bool((self.whole[GUARD + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.whole == FILL).all())


def _all_intact(*bufs):
    return all(b.intact() for b in bufs if b is not None)


def _relmax(got, ref):
    """max |got - ref| / max |ref|, in fp64."""
    ref = ref.double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# =====================================================================================================================================
# 1. points-distribution + xyz loss (dgs_points_loss through losses.points_losses, and directly between guard bands)
# =====================================================================================================================================
# (base, spread, H, W): the depth along each ray is base + spread * rand, the other inputs are those of tests/test_losses._check_points
# (b = 2, v = 3).  The narrow rows are the first 150 steps of configs/diffusionGS_rel.yaml: nearly constant distances per view.
POINTS_ACCURACY = [(1.5, 0.5, 20, 28), (1.5, 0.1, 20, 28), (1.5, 0.02, 20, 28), (1.5, 0.005, 20, 28), (1.5, 0.001, 20, 28),
                   (1.5, 0.02, 128, 128), (4.0, 0.005, 128, 128)]
# (name, b, v, h, w): one pixel (n = 1: torch's unbiased std is NaN there, the kernel's is 0, so the standardised term vanishes and the
# gradient is finite); fewer pixels than the 64 chunks (empty chunks); a size that does not divide; one plane; per-sample weights that
# differ over three samples of two views (a wrong b = bv / V shows)
POINTS_EDGES = [("HW1", 2, 3, 1, 1), ("HW25", 2, 3, 5, 5), ("HW1147", 2, 3, 31, 37), ("B1V1", 1, 1, 9, 13), ("B3V2", 3, 2, 9, 13)]
POINTS_WEIGHTS = [0.7, 1.9, 1.3]
POINTS_W_XYZ = 0.6
POINTS_TOL = 2e-4                      # tests/test_losses.py: loss and gradient
POINTS_FACTOR = 4.0                    # x the error of the reference's torch expression in fp32 (see check_points_accuracy)


def points_inputs(b, v, h, w, base=1.5, spread=0.5):
    g = torch.Generator().manual_seed(11)
    ray_o = (torch.randn(b, v, 3, 1, 1, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 2.0]).reshape(1, 1, 3, 1, 1)).expand(b, v, 3, h, w).contiguous()
    ray_d = F.normalize(torch.randn(b, v, 3, h, w, generator=g), dim=2)
    aligned = ray_o + ray_d * (base + spread * torch.rand(b, v, 1, h, w, generator=g))
    gt = ray_o + ray_d * (1.4 + 0.6 * torch.rand(b, v, 1, h, w, generator=g))
    masks = (torch.rand(b, v, 1, h, w, generator=g) > 0.3).float()
    if not bool(masks.any()):
        masks[0, 0] = 1.0
    return dict(ray_o=ray_o, aligned=aligned, gt=gt, masks=masks, wts=torch.tensor(POINTS_WEIGHTS[:b]))


def points_torch(inp, with_gt, dtype):
    """losses.py:288-292,325-364 as the reference writes them, in `dtype` on the CPU -> (pointsdist [b], xyz, d / d aligned of
    sum_b wts_b pointsdist_b + 0.6 xyz).  One pixel per plane: std = 0 (the kernel's definition; torch's is NaN)."""
    ro, al = inp["ray_o"].to(dtype), inp["aligned"].detach().to(dtype).clone().requires_grad_(True)
    dist = (al - ro).norm(dim=2, p=2, keepdim=True)
    dd = dist.detach()
    std = dd.std(dim=(2, 3, 4), keepdim=True) if dd[0, 0].numel() > 1 else torch.zeros_like(dd[:, :, :1, :1, :1])
    trgt = (dd - dd.mean(dim=(2, 3, 4), keepdim=True)) / (std + 1e-8) * 0.5 + ro.norm(dim=2, p=2, keepdim=True)
    pd = ((dist - trgt) ** 2).mean(dim=(1, 2, 3, 4))
    if with_gt:
        m = inp["masks"].to(dtype)
        xyz = F.mse_loss(al * m, inp["gt"].to(dtype) * m, reduction="sum") / m.sum()
    else:
        xyz = torch.zeros((), dtype=dtype)
    ((pd * inp["wts"].to(dtype)).sum() + POINTS_W_XYZ * xyz).backward()
    return pd.detach(), xyz.detach(), al.grad


def _points_errors(pd, grad, rpd, rgrad):
    """Largest relative error over the samples: of the loss, and of the gradient (max |error| / max |reference| within a sample)."""
    pd, grad = pd.detach().cpu().double(), grad.detach().cpu().double()
    le = float(((pd - rpd.double()).abs() / rpd.double().abs()).max())
    ge = max(float((grad[i] - rgrad[i].double()).abs().max() / rgrad[i].double().abs().max()) for i in range(grad.shape[0]))
    return le, ge


def points_wrapper(lib, device, inp, with_gt):
    from dgs_amd import losses
    al = inp["aligned"].detach().clone().to(device).requires_grad_(True)
    gt, masks = (inp["gt"].to(device), inp["masks"].to(device)) if with_gt else (None, None)
    pd, xyz = losses.points_losses(al, inp["ray_o"].to(device), gt, masks, lib=lib)
    ((pd * inp["wts"].to(device)).sum() + POINTS_W_XYZ * xyz).backward()
    return pd.detach(), xyz.detach(), al.grad


def points_args(lib, device, inp, with_gt):
    """-> (DgsPointsLossArgs for one call giving values and gradient, its guarded outputs (pd, xyz, grad, workspace), the inputs kept
    alive)."""
    L = _lib(lib)
    b, v, _, h, w = inp["aligned"].shape
    al, ro = inp["aligned"].detach().to(device).contiguous(), inp["ray_o"].to(device).contiguous()
    gt, masks = (inp["gt"].to(device).contiguous(), inp["masks"].to(device).contiguous()) if with_gt else (None, None)
    wts = inp["wts"].to(device)
    pd, xyz, grad = Guarded(b, device), Guarded(1, device, init=torch.zeros(1)), Guarded(al.numel(), device)
    ws = Guarded(int(L.dgs_points_loss_workspace_floats(b, v)), device)
    a = _native.DgsPointsLossArgs()
    a.B, a.V, a.H, a.W = b, v, h, w
    a.aligned, a.ray_o, a.gt, a.masks, a.pointsdist, a.xyz = _ptr(al), _ptr(ro), _ptr(gt), _ptr(masks), _ptr(pd.t), _ptr(xyz.t)
    a.w_pointsdist, a.w_xyz, a.grad, a.workspace = _ptr(wts), POINTS_W_XYZ if with_gt else 0.0, _ptr(grad.t), _ptr(ws.t)
    return a, (pd, xyz, grad, ws), (al, ro, gt, masks, wts)


def points_guarded(lib, device, inp, with_gt):
    """dgs_points_loss itself, every output and the workspace between guard bands."""
    a, (pd, xyz, grad, ws), keep = points_args(lib, device, inp, with_gt)
    assert _lib(lib).dgs_points_loss(ctypes.byref(a), _stream(device)) == 0
    assert _all_intact(pd, xyz, grad, ws), "dgs_points_loss wrote outside its outputs or its workspace"
    return pd.t, xyz.t[0], grad.t.view(keep[0].shape)


def measure_points_accuracy(lib, device, cases=POINTS_ACCURACY):
    """-> [(case name, (kernel loss error, gradient error), (fp32 torch loss error, gradient error))] against fp64, without a gt (the
    points-distribution term alone, as in the steps where nothing else is active)."""
    out = []
    for base, spread, h, w in cases:
        inp = points_inputs(2, 3, h, w, base, spread)
        rpd, _, rgrad = points_torch(inp, False, torch.float64)
        tpd, _, tgrad = points_torch(inp, False, torch.float32)
        pd, _, grad = points_wrapper(lib, device, inp, False)
        std = float((inp["aligned"] - inp["ray_o"]).detach().double().norm(dim=2).reshape(6, -1).std(dim=1).mean())
        out.append((f"{base}, {spread}, {h}x{w}", std, _points_errors(pd, grad, rpd, rgrad), _points_errors(tpd, tgrad, rpd, rgrad)))
    return out


def check_points_accuracy(lib, device):
    """Loss and gradient, separately, within max(2e-4, 4 x the error of the reference's own torch expression evaluated in fp32 on the CPU
    on the same inputs against the same fp64).  4: sums of the shifted distances sit at 0.3 - 1.6 x that error, which leaves 2.5 x for
    another summation order and the GPU's FMA contraction; sums of the raw distances and their squares are 80 - 600 x off at the narrow
    spreads (profiles/step_kernels_parity.txt)."""
    failed = []
    for name, _, kernel, torch32 in measure_points_accuracy(lib, device):
        for what, k, t in zip(("loss", "gradient"), kernel, torch32):
            bar = max(POINTS_TOL, POINTS_FACTOR * t)
            record("points loss", name, what, k, t, bar)
            print(f"points loss {name:22s} {what:8s} kernel {k:.3e} fp32 torch {t:.3e} bar {bar:.3e}")
            if not k <= bar:
                failed.append((name, what, k, bar))
    assert not failed, failed


def check_points_edges(lib, device):
    """Shape edges with and without gt and masks at the tolerances of tests/test_losses.py, through the wrapper; the direct call between
    guard bands gives the same bits (fixed reduction order)."""
    for name, b, v, h, w in POINTS_EDGES:
        inp = points_inputs(b, v, h, w)
        for with_gt in (True, False):
            rpd, rxyz, rgrad = points_torch(inp, with_gt, torch.float64)
            pd, xyz, grad = points_wrapper(lib, device, inp, with_gt)
            tag = (name, with_gt)
            assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(pd).all()), tag
            assert torch.allclose(pd.cpu().double(), rpd, rtol=POINTS_TOL), (tag, pd, rpd)
            assert torch.allclose(xyz.cpu().double(), rxyz, rtol=1e-5, atol=1e-12), (tag, xyz, rxyz)
            gerr = _relmax(grad, rgrad)
            assert gerr < POINTS_TOL, (tag, gerr)
            record("points loss edges", f"{name} gt={int(with_gt)}", "gradient", gerr, None, POINTS_TOL)
            pd2, xyz2, grad2 = points_guarded(lib, device, inp, with_gt)
            assert torch.equal(pd2, pd) and torch.equal(xyz2, xyz) and torch.equal(grad2, grad), tag
            if h * w == 1:                                 # n = 1: std 0, the standardised term is 0, so the target is |ray_o|
                d, o = (inp["aligned"] - inp["ray_o"]).double().norm(dim=2), inp["ray_o"].double().norm(dim=2)
                assert torch.allclose(pd.cpu().double(), ((d - o) ** 2).mean(dim=(1, 2, 3)), rtol=POINTS_TOL), tag


# =====================================================================================================================================
# 2. MSE / PSNR (dgs_mse_psnr through losses.mse_psnr / losses.compute_psnr, and directly between guard bands)
# =====================================================================================================================================
# n per sample: 12 (3 float4: fewer than the 64 chunks), 108, 300, 3672, 49152
MSE_SHAPES = [(1, 1, 3, 2, 2), (1, 1, 3, 6, 6), (2, 1, 3, 10, 10), (3, 2, 3, 34, 18), (1, 4, 3, 64, 64)]


def mse_guarded(lib, device, render, target, clamp01, grad_scale, expect_ok=True):
    L = _lib(lib)
    r, t = render.to(device).contiguous(), target.to(device).contiguous()
    B, n = r.shape[0], r[0].numel()
    l2, psnr, grad, partial = Guarded(B, device), Guarded(B, device), Guarded(r.numel(), device), Guarded(B * _native.LOSS_CHUNKS, device)
    a = _native.DgsMseArgs()
    a.B, a.n, a.rendering, a.target, a.clamp01 = B, n, _ptr(r), _ptr(t), int(clamp01)
    a.l2, a.psnr, a.grad, a.grad_scale, a.partial = _ptr(l2.t), _ptr(psnr.t), _ptr(grad.t), float(grad_scale), _ptr(partial.t)
    rc = L.dgs_mse_psnr(ctypes.byref(a), _stream(device))
    if not expect_ok:
        assert rc != 0
        assert all(x.untouched() for x in (l2, psnr, grad, partial)), "a refused dgs_mse_psnr wrote something"
        return None
    assert rc == 0
    assert _all_intact(l2, psnr, grad, partial), "dgs_mse_psnr wrote outside its outputs"
    return l2.t, psnr.t, grad.t.view(r.shape)


def check_mse(lib, device):
    from dgs_amd import losses
    # -- exact: target = 0, rendering[b] = 2^b -> every sum is an integer multiple of 4^b below 2^24 of them, l2[b] = 4^b, and the
    #    gradient is fl(fl(grad_scale * 2) / n) * 2^b per element; one dropped or doubled float4 breaks the equality
    for shape in [(4, 1, 3, 2, 2), (4, 1, 3, 6, 6), (4, 2, 3, 34, 18), (3, 4, 3, 64, 64)]:
        B, n = shape[0], int(np.prod(shape[1:]))
        render = (2.0 ** torch.arange(B, dtype=torch.float32)).reshape(B, 1, 1, 1, 1).expand(shape).contiguous()
        target = torch.zeros(shape)
        want_l2 = 4.0 ** torch.arange(B, dtype=torch.float32)
        for gs in (1.0 / B, 0.37):
            l2, psnr, grad = mse_guarded(lib, device, render, target, False, gs)
            assert torch.equal(l2.cpu(), want_l2), (shape, l2)
            k = torch.tensor(gs, dtype=torch.float32) * 2.0 / torch.tensor(float(n), dtype=torch.float32)
            assert torch.equal(grad.cpu(), k * render), shape
            assert torch.allclose(psnr.cpu().double(), -10.0 * torch.log10(want_l2.double()), rtol=1e-5, atol=1e-5), shape
        r = render.clone().to(device).requires_grad_(True)
        loss, l2, _ = losses.mse_psnr(r, target.to(device), lib=lib)
        loss.backward()
        assert torch.equal(l2.detach().cpu(), want_l2), shape
        assert torch.equal(r.grad.cpu(), (torch.tensor(1.0 / B, dtype=torch.float32) * 2.0 / torch.tensor(float(n), dtype=torch.float32)) * render), shape
    # -- random values against fp64 at the tolerances of tests/test_losses.py; inputs outside [0, 1] on both sides for clamp01
    g = torch.Generator().manual_seed(5)
    for shape in MSE_SHAPES:
        B, V = shape[:2]
        render = torch.rand(shape, generator=g) * 1.4 - 0.2
        target = torch.rand(shape, generator=g) * 1.2 - 0.1
        wts = torch.tensor([1.0, 0.0, 2.0][:B])
        r = render.clone().to(device).requires_grad_(True)
        loss, l2, psnr = losses.mse_psnr(r, target.to(device), lib=lib)
        (0.7 * loss + (l2 * wts.to(device)).sum()).backward()
        rr = render.clone().double().requires_grad_(True)
        rl2 = ((rr - target.double()) ** 2).mean(dim=(1, 2, 3, 4))
        (0.7 * rl2.mean() + (rl2 * wts.double()).sum()).backward()
        assert torch.allclose(l2.detach().cpu().double(), rl2.detach(), rtol=2e-6), shape
        assert torch.allclose(psnr.cpu().double(), -10.0 * torch.log10(rl2.detach()), rtol=1e-5, atol=1e-5), shape
        assert torch.allclose(loss.detach().cpu().double(), rl2.detach().mean(), rtol=2e-6), shape
        assert torch.allclose(r.grad.cpu().double(), rr.grad, rtol=1e-5, atol=1e-9), shape
        record("mse", str(shape), "l2", float(((l2.detach().cpu().double() - rl2.detach()).abs() / rl2.detach()).max()), None, 2e-6)
        l2g, psnrg, gradg = mse_guarded(lib, device, render, target, False, 1.0 / B)       # the same bits between guard bands
        assert torch.equal(l2g, l2.detach()) and torch.equal(psnrg, psnr)
        gr = (2.0 / (B * rr[0].numel())) * (render.double() - target.double())
        assert torch.allclose(gradg.cpu().double(), gr, rtol=1e-5, atol=1e-9), shape
        # compute_psnr: clamp to [0, 1], per image
        img_r, img_t = render.reshape(B * V, *shape[2:]), target.reshape(B * V, *shape[2:])
        want = -10.0 * torch.log10(((img_t.double().clamp(0, 1) - img_r.double().clamp(0, 1)) ** 2).mean(dim=(1, 2, 3)))
        got = losses.compute_psnr(img_t.to(device), img_r.to(device), lib=lib)
        assert torch.allclose(got.cpu().double(), want, rtol=1e-5, atol=1e-5), shape
        l2c, _, gradc = mse_guarded(lib, device, img_r, img_t, True, 1.0)
        d = img_r.double().clamp(0, 1) - img_t.double().clamp(0, 1)
        assert torch.allclose(l2c.cpu().double(), (d ** 2).mean(dim=(1, 2, 3)), rtol=2e-6), shape
        assert torch.allclose(gradc.cpu().double(), 2.0 * d / d[0].numel(), rtol=1e-5, atol=1e-9), shape      # as the kernel defines it: of the clamped difference
    # -- n = 27 is no multiple of 4: refused, nothing written
    bad = torch.rand(2, 1, 3, 3, 3, generator=g)
    mse_guarded(lib, device, bad, bad * 0.5, False, 1.0, expect_ok=False)
    with torch.no_grad():
        try:
            losses.mse_psnr(bad.to(device), (bad * 0.5).to(device), lib=lib)
        except RuntimeError:
            pass
        else:
            raise AssertionError("mse_psnr accepted n = 27")


# =====================================================================================================================================
# 3. the LPIPS input resize (dgs_resize_bilinear[_backward] through losses.lpips_input, and directly between guard bands)
# =====================================================================================================================================
# (leading dims, (in_h, in_w), (out_h, out_w)).  Every in / out ratio is a dyadic fraction with a small numerator, so the source
# coordinate (dst + 0.5) * in / out - 0.5 is exact in fp32 and the fp64 interpolation is a reference at the same 2e-6 as the fp32 one
# (ratios that round are compared with fp32 torch in tests/test_losses.py: 300 x 200 -> 256 x 256).
RESIZE_CASES = [((1, 3), (1, 1), (256, 256)),          # in - 1 = 0: both neighbours clamp to the one pixel
                ((1, 3), (2, 3), (256, 256)),          # clamp at both ends of two- and three-pixel rows
                ((1, 2), (257, 255), (256, 256)),      # odd downsample, one side just above, one just below
                ((1, 1), (1024, 768), (256, 256)),     # factors 4 and 3: input pixels that feed no output
                ((7,), (20, 14), (5, 7)),              # 245 outputs: below one workgroup
                ((2, 3), (80, 72), (32, 48))]          # non-square output, factors 2.5 and 1.5


def resize_guarded(lib, device, x, size, ddst=None):
    L = _lib(lib)
    x = x.to(device).contiguous()
    planes = int(np.prod(x.shape[:-2]))
    a = _native.DgsResizeArgs()
    a.planes, a.in_h, a.in_w, a.out_h, a.out_w = planes, int(x.shape[-2]), int(x.shape[-1]), int(size[0]), int(size[1])
    a.mul, a.add = 2.0, -1.0
    if ddst is None:
        dst = Guarded(planes * size[0] * size[1], device)
        a.src, a.dst = _ptr(x), _ptr(dst.t)
        assert L.dgs_resize_bilinear(ctypes.byref(a), _stream(device)) == 0
        assert dst.intact(), "dgs_resize_bilinear wrote outside its output"
        return dst.t.view(*x.shape[:-2], *size)
    ddst = ddst.to(device).contiguous()
    dsrc = Guarded(x.numel(), device)
    a.ddst, a.dsrc = _ptr(ddst), _ptr(dsrc.t)
    assert L.dgs_resize_bilinear_backward(ctypes.byref(a), _stream(device)) == 0
    assert dsrc.intact(), "dgs_resize_bilinear_backward wrote outside its output"
    return dsrc.t.view(x.shape)


def check_resize(lib, device):
    from dgs_amd import losses
    g = torch.Generator().manual_seed(9)
    for lead, (h, w), size in RESIZE_CASES:
        x = torch.rand(*lead, h, w, generator=g)
        batched = lambda t: t if t.dim() == 4 else t.unsqueeze(0)
        xd = x.clone().to(device).requires_grad_(True)
        y = losses.lpips_input(xd, size=size, lib=lib)
        assert y.shape == (*lead, *size)
        wgt = torch.randn(y.shape, generator=g)
        (y * wgt.to(device)).sum().backward()
        tag = (h, w, size)
        for dtype in (torch.float32, torch.float64):
            xr = x.clone().to(dtype).requires_grad_(True)
            ref = (F.interpolate(batched(xr), size=list(size), mode="bilinear") * 2.0 - 1.0).reshape(y.shape)
            (ref * wgt.to(dtype)).sum().backward()
            err = float((y.detach().cpu().double() - ref.detach().double()).abs().max())
            record("resize", f"{h}x{w} -> {size[0]}x{size[1]}", f"value vs {str(dtype)[6:]}", err, None, 2e-6)
            assert err <= 2e-6, (tag, dtype, err)
            gmax = float(xr.grad.abs().max())
            assert torch.allclose(xd.grad.cpu().double(), xr.grad.double(), rtol=1e-4, atol=1e-5 * gmax), (tag, dtype)
        assert torch.equal(resize_guarded(lib, device, x, size), y.detach()), tag                    # same bits between guard bands
        dx = resize_guarded(lib, device, x, size, ddst=wgt)
        assert torch.allclose(dx.cpu().double(), xr.grad.double(), rtol=1e-4, atol=1e-5 * gmax), tag


# =====================================================================================================================================
# 4. sum of squares (dgs_sumsq_partials / dgs_sumsq_finish directly, and through parallel.GradNorm)
# =====================================================================================================================================
SUMSQ_CHUNK = 65536
SUMSQ_NS = [1, 3, 4, 5, 1023, 1024, 1027, 65535, 65536, 65537, 2 * 65536 + 1030]
SUMSQ_HOT = [0, 3, 1023, 1024, 65535, 65536]           # and n - 1
# per lane 256 sequential fp32 additions, then 6 shuffle steps and 3 additions, all on non-negative terms
SUMSQ_BAR = 265.0 * 2.0 ** -24


def sumsq_guarded(lib, device, x, n, finish=True):
    """x: device tensor of at least n elements -> (partials [count], total [1] or None), both between guard bands."""
    L = _lib(lib)
    count = int(L.dgs_sumsq_count(n))
    assert count == -(-n // SUMSQ_CHUNK)
    partials, total = Guarded(count, device), Guarded(1, device)
    assert L.dgs_sumsq_partials(_ptr(x), n, _ptr(partials.t), _stream(device)) == 0
    if finish:
        assert L.dgs_sumsq_finish(_ptr(partials.t), count, _ptr(total.t), _stream(device)) == 0
    assert _all_intact(partials, total), "the sum of squares wrote outside its outputs"
    return partials.t, (total.t if finish else None)


def _chunk_sizes(n):
    return torch.tensor([min(SUMSQ_CHUNK, n - c * SUMSQ_CHUNK) for c in range(-(-n // SUMSQ_CHUNK))], dtype=torch.float32)


def check_sumsq(lib, device):
    L = _lib(lib)
    g = torch.Generator().manual_seed(21)
    worst = 0.0
    for n in SUMSQ_NS:
        # all ones: every partial is its element count, the total is n, exactly
        partials, total = sumsq_guarded(lib, device, torch.ones(n, device=device), n)
        assert torch.equal(partials.cpu(), _chunk_sizes(n)), (n, partials)
        assert float(total[0]) == float(n), (n, total)
        # one hot: that chunk's partial is 9, every other one 0
        x = torch.zeros(n, device=device)
        for i in sorted(set(h for h in SUMSQ_HOT + [n - 1] if h < n)):
            x[i] = 3.0
            partials, total = sumsq_guarded(lib, device, x, n)
            want = torch.zeros(partials.numel())
            want[i // SUMSQ_CHUNK] = 9.0
            assert torch.equal(partials.cpu(), want), (n, i, partials)
            assert float(total[0]) == 9.0, (n, i)
            x[i] = 0.0
        # random: each partial, and the total, against fp64 of its own elements
        x = torch.randn(n, generator=g)
        partials, total = sumsq_guarded(lib, device, x.to(device), n)
        ref = torch.stack([c.double().pow(2).sum() for c in x.split(SUMSQ_CHUNK)])
        err = float(((partials.cpu().double() - ref).abs() / ref).max())
        terr = float((total.cpu().double()[0] - ref.sum()).abs() / ref.sum())
        worst = max(worst, err, terr)
        assert err <= SUMSQ_BAR and terr <= SUMSQ_BAR, (n, err, terr)
    record("sumsq", "all n", "partials and totals", worst, None, SUMSQ_BAR)
    print(f"sum of squares: worst relative error {worst:.3e}, bar {SUMSQ_BAR:.3e}")
    # the full-chunk form and the tail form add in the same order: the same bits
    x = torch.randn(SUMSQ_CHUNK, generator=g)
    x[-1] = 0.0
    xd = x.to(device)
    full, _ = sumsq_guarded(lib, device, xd, SUMSQ_CHUNK, finish=False)
    tail, _ = sumsq_guarded(lib, device, xd, SUMSQ_CHUNK - 1, finish=False)
    assert torch.equal(full, tail), (full, tail)
    # GradNorm: buckets in any order; a partial is written, not accumulated
    from dgs_amd.parallel import GradNorm
    n = SUMSQ_NS[-1]
    flat = torch.randn(n, generator=g).to(device)
    gn = GradNorm(flat, L)
    gp, gt_ = Guarded(gn.count, device), Guarded(1, device)
    gn.partials, gn.sumsq = gp.t, gt_.t
    for a, b in ((2 * SUMSQ_CHUNK, n), (0, SUMSQ_CHUNK), (SUMSQ_CHUNK, 2 * SUMSQ_CHUNK)):
        gn.add(a, b)
    partials, total = sumsq_guarded(lib, device, flat, n)
    assert torch.equal(gn.total(), total) and torch.equal(gn.partials, partials)
    flat[SUMSQ_CHUNK:2 * SUMSQ_CHUNK] *= 2.0
    gn.add(SUMSQ_CHUNK, 2 * SUMSQ_CHUNK)
    gn.add(SUMSQ_CHUNK, 2 * SUMSQ_CHUNK)
    partials2, total2 = sumsq_guarded(lib, device, flat, n)
    assert torch.equal(gn.total(), total2) and torch.equal(gn.partials, partials2)
    assert float(partials2[1]) == 4.0 * float(partials[1]) and float(partials2[0]) == float(partials[0])
    assert _all_intact(gp, gt_)
    # refusals: nothing is written
    xs = torch.ones(64, device=device)
    p, t = Guarded(1, device), Guarded(1, device)
    st = _stream(device)
    assert L.dgs_sumsq_partials(None, 8, _ptr(p.t), st) != 0 and L.dgs_sumsq_partials(_ptr(xs), 8, None, st) != 0
    assert L.dgs_sumsq_partials(_ptr(xs), 0, _ptr(p.t), st) != 0 and L.dgs_sumsq_partials(_ptr(xs), -5, _ptr(p.t), st) != 0
    assert xs.data_ptr() % 16 == 0
    assert L.dgs_sumsq_partials(ctypes.c_void_p(xs.data_ptr() + 4), 8, _ptr(p.t), st) != 0          # x not 16-byte aligned
    assert L.dgs_sumsq_finish(None, 1, _ptr(t.t), st) != 0 and L.dgs_sumsq_finish(_ptr(p.t), 1, None, st) != 0
    assert L.dgs_sumsq_finish(_ptr(p.t), 0, _ptr(t.t), st) != 0
    assert L.dgs_sumsq_count(0) == 0 and L.dgs_sumsq_count(-1) == 0
    assert p.untouched() and t.untouched()


# =====================================================================================================================================
# 5. AdamW + copies at table level (dgs_adamw_step, and dgs_adamw_ema_step as its twin)
# =====================================================================================================================================
BF, F32 = torch.bfloat16, torch.float32
# (rows, cols, copy dtype or None, transposed copy), flat and block entries interleaved.  numel 1, 3, 14: the scalar tail; 4095: the
# scalar tail across the tile's end; 4096: one full float4 tile; 4097: the scalar tail over two tiles; 4100: the float4 path with a
# 4-element last tile; 8200, 3 * 4096: several tiles; 64 x 128 with a bf16 copy: flat; the transposed ones: 1, 2 x 3 and 3 x 1 blocks
ADAMW_TABLE = [(1, 1, None, False), (64, 64, BF, True), (1, 3, F32, False), (1, 4095, BF, False), (128, 192, BF, True), (1, 14, BF, False),
               (1, 4096, F32, False), (1, 4097, None, False), (192, 64, BF, True), (1, 4100, BF, False), (1, 8200, F32, False),
               (64, 128, BF, False), (1, 3 * 4096, BF, False)]
ADAMW_LR, ADAMW_BETAS, ADAMW_EPS = 3e-2, (0.9, 0.99), 1e-8
ADAMW_STEPS = (1, 2, 3, 10000)
ADAMW_DECAYS = (0.0, 0.05)
# (name, max_grad_norm): off -- a NaN sits in the sum-of-squares word and must be ignored; the gradient norm of the table is ~ 230, so
# 0.5 clips and 1000 does not
ADAMW_CLIPS = (("off", 0.0), ("above", 0.5), ("below", 1000.0))
ADAMW_EMA_DECAY = 0.9


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adamw_ref64(p, g, m, v, sumsq, step, wd, max_norm):
    """adamw_hyper, clip_coef and adamw_one of csrc/optim.hip written out in fp64 on the fp32 inputs and the fp32-rounded arguments."""
    lr, b1, b2, eps, wd = _f32(ADAMW_LR), _f32(ADAMW_BETAS[0]), _f32(ADAMW_BETAS[1]), _f32(ADAMW_EPS), _f32(wd)
    bc1, bc2s = _f32(1.0 - ADAMW_BETAS[0] ** step), _f32((1.0 - ADAMW_BETAS[1] ** step) ** 0.5)
    gc = 1.0
    if max_norm > 0.0:
        gc = min(1.0, _f32(max_norm) / (float(sumsq) ** 0.5 + _f32(1.0e-6)))
    p, g, m, v = p.double(), g.double() * gc, m.double(), v.double()
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + ((1.0 - b2) * g) * g
    p = p - (lr / bc1) * (m / (v.sqrt() * (1.0 / bc2s) + eps))
    return p, m, v


def adamw_torch32(p, g, m, v, sumsq, step, wd, max_norm):
    """torch.optim.AdamW (foreach=False, fused=False) in fp32 on the CPU, one step from the same state, the gradient pre-multiplied by the
    fp32 clip coefficient."""
    gc = torch.ones((), dtype=torch.float32)
    if max_norm > 0.0:
        gc = (torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(float(sumsq), dtype=torch.float32).sqrt() + 1e-6)).clamp(max=1.0)
    q = torch.nn.Parameter(p.clone())
    q.grad = g * gc
    opt = torch.optim.AdamW([q], lr=ADAMW_LR, betas=ADAMW_BETAS, eps=ADAMW_EPS, weight_decay=wd, foreach=False, fused=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


class AdamWState:
    """The table's tensors: p, m, v (and the EMA shadows) as slices of flat buffers laid out by optim.flat_offsets, 7.0 in the padding
    between the slices and in a band on either side; every copy in a guarded buffer of its own."""

    def __init__(self, lib, device, P, M, V):
        from dgs_amd.optim import flat_offsets
        self.lib, self.dev = _lib(lib), device
        self.offs, self.total = flat_offsets(r * c for r, c, _, _ in ADAMW_TABLE)
        self.flat = {k: Guarded(self.total, device) for k in ("p", "m", "v", "ema", "g")}
        self.pad = torch.ones(self.total, dtype=torch.bool)
        for (r, c, _, _), off in zip(ADAMW_TABLE, self.offs):
            self.pad[off:off + r * c] = False
        self.pad = self.pad.to(device)
        self.copy, self.copy_t = [], []
        for i, ((r, c, kind, tr), off) in enumerate(zip(ADAMW_TABLE, self.offs)):
            for k, src in (("p", P), ("m", M), ("v", V), ("ema", P)):
                self.view(k, i).copy_(src[i])
            self.copy.append(None if kind is None else Guarded(r * c, device, dtype=kind))
            self.copy_t.append(Guarded(r * c, device, dtype=BF) if tr else None)
        entries = []
        for i, ((r, c, kind, tr), off) in enumerate(zip(ADAMW_TABLE, self.offs)):
            t = _native.DgsAdamWTensor()
            t.p, t.g, t.m, t.v = (self.view(k, i).data_ptr() for k in ("p", "g", "m", "v"))
            t.rows, t.cols = r, c
            if kind is not None:
                t.copy, t.copy_kind = self.copy[i].t.data_ptr(), _native.OPTIM_COPY_BF16 if kind == BF else _native.OPTIM_COPY_F32
            if tr:
                t.copy_t = self.copy_t[i].t.data_ptr()
            entries.append(t)
        host = (_native.DgsAdamWTensor * len(entries))(*entries)
        self.n_tiles = int(self.lib.dgs_adamw_plan(host, len(entries)))
        want = sum((r // 64) * (c // 64) if tr else -(-r * c // 4096) for r, c, _, tr in ADAMW_TABLE)
        assert self.n_tiles == want, (self.n_tiles, want)
        self.table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
        self.sumsq = Guarded(1, device)

    def view(self, k, i):
        r, c, _, _ = ADAMW_TABLE[i]
        return self.flat[k].t[self.offs[i]:self.offs[i] + r * c].view(r, c)

    def set_grads(self, G):
        for i, gr in enumerate(G):
            self.view("g", i).copy_(gr)

    def step(self, step, wd, max_norm, ema=False):
        a = _native.DgsAdamWArgs()
        a.tensors, a.n_tensors, a.n_tiles = self.table.data_ptr(), len(ADAMW_TABLE), self.n_tiles
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = ADAMW_LR, ADAMW_BETAS[0], ADAMW_BETAS[1], ADAMW_EPS, wd
        a.bias_correction1, a.bias_correction2_sqrt = 1.0 - ADAMW_BETAS[0] ** step, (1.0 - ADAMW_BETAS[1] ** step) ** 0.5
        a.grad_sumsq, a.max_grad_norm = self.sumsq.t.data_ptr(), max_norm
        if ema:
            f = _native.DgsEmaFusedArgs()
            f.ema_base, f.m_base, f.one_minus_decay = self.flat["ema"].t.data_ptr(), self.flat["m"].t.data_ptr(), 1.0 - ADAMW_EMA_DECAY
            assert self.lib.dgs_adamw_ema_step(ctypes.byref(a), ctypes.byref(f), _stream(self.dev)) == 0
        else:
            assert self.lib.dgs_adamw_step(ctypes.byref(a), _stream(self.dev)) == 0

    def guards_ok(self, ema):
        for k in ("p", "m", "v", "ema", "g"):
            f = self.flat[k]
            assert f.intact() and bool((f.t[self.pad] == FILL).all()), f"AdamW wrote outside the slices of its {k} buffer"
        assert _all_intact(self.sumsq, *self.copy, *self.copy_t), "AdamW wrote outside a copy"
        if not ema:
            assert all(torch.equal(self.view("ema", i), self.ema0[i]) for i in range(len(ADAMW_TABLE))), "dgs_adamw_step touched the shadows"

    def snapshot(self):
        return ([self.flat[k].whole.clone() for k in ("p", "m", "v", "ema")] + [None if c is None else c.whole.clone() for c in self.copy + self.copy_t])

    def copies_follow(self, tag):
        for i, (r, c, kind, tr) in enumerate(ADAMW_TABLE):
            p = self.view("p", i)
            if kind is not None:
                cp = self.copy[i].t.view(r, c)
                assert torch.equal(cp, p.to(kind)), (tag, ADAMW_TABLE[i], "copy")
                if tr:
                    assert torch.equal(self.copy_t[i].t.view(c, r), cp.t()), (tag, ADAMW_TABLE[i], "transposed copy")


def check_adamw(lib, device):
    g = torch.Generator().manual_seed(31)
    shapes = [(r, c) for r, c, _, _ in ADAMW_TABLE]
    # every tensor holds data of its own (a wrong first_tile lookup lands on another tensor's values): scales that differ per tensor
    P0 = [torch.randn(s, generator=g) * (0.5 + 0.25 * i) for i, s in enumerate(shapes)]
    M0 = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    V0 = [torch.rand(s, generator=g) * 0.02 + 1e-3 for s in shapes]
    for wd in ADAMW_DECAYS:
        for clip, max_norm in ADAMW_CLIPS:
            st, twin = AdamWState(lib, device, P0, M0, V0), AdamWState(lib, device, P0, M0, V0)
            for step in ADAMW_STEPS:
                G = [torch.randn(s, generator=g) * (1.0 + 0.1 * i) for i, s in enumerate(shapes)]
                sumsq = float(sum(x.double().pow(2).sum() for x in G).float())
                assert (sumsq ** 0.5 > max_norm) == (clip != "below")
                for s in (st, twin):
                    s.set_grads(G)
                    s.sumsq.t.fill_(float("nan") if clip == "off" else sumsq)
                    s.ema0 = [s.view("ema", i).clone() for i in range(len(shapes))]
                before = [[st.view(k, i).cpu().clone() for i in range(len(shapes))] for k in ("p", "m", "v")]
                st.step(step, wd, max_norm)
                twin.step(step, wd, max_norm, ema=True)
                tag = (wd, clip, step)
                st.guards_ok(False)
                twin.guards_ok(True)
                for i, shape in enumerate(ADAMW_TABLE):
                    args = (before[0][i], G[i], before[1][i], before[2][i], sumsq, step, wd, max_norm)
                    ref, t32 = adamw_ref64(*args), adamw_torch32(*args)
                    for k, r, t in zip(("p", "m", "v"), ref, t32):
                        got = st.view(k, i).cpu().double()
                        err, terr, top = float((got - r).abs().max()), float((t.double() - r).abs().max()), float(r.abs().max())
                        bar = max(4.0 * terr, 2.0 ** -23 * top)
                        record("adamw", f"wd={wd} clip={clip} step={step} {shape[0]}x{shape[1]}", k, err, terr, bar)
                        assert err <= bar, (tag, shape, k, err, terr, bar)
                        assert err <= 2e-6 * top, (tag, shape, k, err, top)
                        assert torch.equal(st.view(k, i), twin.view(k, i)), (tag, shape, k, "dgs_adamw_ema_step moved the update")
                    # the shadow of the new value, the reference's expression (utils/ema.py:94-101) bit for bit
                    want = twin.ema0[i].clone()
                    diff = want - twin.view("p", i)
                    diff.mul_(1.0 - ADAMW_EMA_DECAY)
                    want.sub_(diff)
                    assert torch.equal(twin.view("ema", i), want), (tag, shape, "shadow")
                st.copies_follow(tag)
                twin.copies_follow(tag)
            # a sum of squares that is not finite, the clip on: nothing is touched
            for bad in (float("nan"), float("inf"), float("-inf")):
                for s, ema in ((st, False), (twin, True)):
                    keep = s.snapshot()
                    s.sumsq.t.fill_(bad)
                    s.step(4, wd, 0.5, ema=ema)
                    now = s.snapshot()
                    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(keep, now)), (wd, clip, bad, ema)
                    assert s.sumsq.intact()


# =====================================================================================================================================
# 6. sampler step (dgs_sampler_step directly, and through SpacedDiffusion.step)
# =====================================================================================================================================
# the kernel's grid is capped at 1024 workgroups of 256 lanes, one float4 each: 1024 * 256 + 257 float4 per sample take a full first
# trip and a second one of one workgroup and one lane.  [B, V, 3, 188, 1861] with V = 2: one predicted view of 3 * 188 * 1861 elements
SAMPLER_PER = 4 * (1024 * 256 + 257)
SAMPLER_VIEW = (3, 188, 1861)
SAMPLER_B = 3
assert int(np.prod(SAMPLER_VIEW)) == SAMPLER_PER

_sampler_cache = {}


def sampler_data():
    """Shared by the sampler checks and left unchanged: model output with values outside [-1, 1], x_t, noise (CPU, fp32)."""
    if not _sampler_cache:
        g = torch.Generator().manual_seed(41)
        _sampler_cache["render"] = torch.randn(SAMPLER_B, 2, *SAMPLER_VIEW, generator=g) * 0.8
        _sampler_cache["x_t"] = torch.randn(SAMPLER_B, 1, *SAMPLER_VIEW, generator=g)
        _sampler_cache["noise"] = torch.randn(SAMPLER_B, 1, *SAMPLER_VIEW, generator=g)
    return _sampler_cache


def sampler_expected(d, data, t, clip, with_noise=True):
    """The reference's expression (gaussian_diffusion.py:301-304, 504-512) in fp32 torch on the CPU with the coefficient tensors read back
    from the SpacedDiffusion object: c1 * x0 + c2 * x, then + sigma * z where t != 0."""
    c1, c2, sg = d._coef1.cpu(), d._coef2.cpu(), d._sigma.cpu()
    x0 = data["render"][:, 1:]
    x0 = x0.clamp(-1.0, 1.0) if clip else x0.clone()
    out = torch.empty_like(data["x_t"])
    for b, tb in enumerate(t):
        mean = c1[tb] * x0[b] + c2[tb] * data["x_t"][b]
        out[b] = mean + sg[tb] * data["noise"][b] if (tb != 0 and with_noise) else mean
    return out, x0


def sampler_call(lib, device, d, model, x_t, noise, t, clip, out, pred, bad_t, per=SAMPLER_PER, offset=SAMPLER_PER, stride=2 * SAMPLER_PER, B=SAMPLER_B):
    a = _native.DgsSamplerStepArgs()
    a.B, a.per_sample, a.model_stride, a.model_offset = B, per, stride, offset
    a.model_output, a.x_t, a.noise, a.t = _ptr(model), _ptr(x_t), _ptr(noise), _ptr(t)
    a.coef1, a.coef2, a.sigma, a.T = _ptr(d._coef1), _ptr(d._coef2), _ptr(d._sigma), d.num_timesteps
    a.clip_denoised, a.out, a.pred_xstart, a.bad_t = int(clip), _ptr(out), _ptr(pred), _ptr(bad_t)
    return _lib(lib).dgs_sampler_step(ctypes.byref(a), _stream(device))


def check_sampler_step(lib, device):
    """SpacedDiffusion.step at t = [0, T - 1, 7] with predicted_views_offset = 1 (a non-zero model offset): bit-equal to the fp32 torch
    expression -- sampler.hip is built without contraction and claims the reference's order -- and within 2e-6 of the numpy oracle.
    Clip on with pred_xstart into a buffer of its own; clip off, in place (out = x_t)."""
    from dgs_amd import sampler
    from oracle import sampler_oracle as so
    d = sampler.create_diffusion("30", device=device, lib=lib)
    tab = so.Tables("30")
    T = d.num_timesteps
    data = sampler_data()
    ts = [0, T - 1, 7]
    t = torch.tensor(ts, dtype=torch.int64, device=device)
    render, noise = data["render"].to(device), data["noise"].to(device)
    for clip, in_place in ((True, False), (False, True)):
        want, want_x0 = sampler_expected(d, data, ts, clip)
        x = Guarded(SAMPLER_B * SAMPLER_PER, device, init=data["x_t"])
        x_t = x.t.view(data["x_t"].shape)
        if in_place:
            out, pred = x, None
            got = d.step(render, x_t, t, noise=noise, clip_denoised=clip, out=x_t, predicted_views_offset=1)
            assert got.data_ptr() == x_t.data_ptr()
        else:
            out, pred = Guarded(SAMPLER_B * SAMPLER_PER, device), Guarded(SAMPLER_B * SAMPLER_PER, device)
            got = d.step(render, x_t, t, noise=noise, clip_denoised=clip, out=out.t.view(x_t.shape), pred_xstart=pred.t.view(x_t.shape),
                         predicted_views_offset=1)
            assert torch.equal(x_t.cpu(), data["x_t"])                                       # x_t is read, never written
            assert torch.equal(pred.t.view(x_t.shape).cpu(), want_x0), "pred_xstart is not the (clipped) model output"
        assert _all_intact(x, out, pred), "dgs_sampler_step wrote outside its outputs"
        got = got.cpu()
        nbad = int((got != want).sum())
        assert nbad == 0, (clip, in_place, nbad, float((got - want).abs().max()))
        for b, tb in enumerate(ts):
            o, x0 = so.p_sample(tab, data["render"][b:b + 1].numpy(), data["x_t"][b:b + 1].numpy(), tb, data["noise"][b:b + 1].numpy(), clip_denoised=clip)
            np.testing.assert_allclose(got[b:b + 1].numpy(), o, rtol=2e-6, atol=2e-6)
    assert (want_x0.abs() > 1.0).any()                     # the unclipped run really carried values outside [-1, 1]


def check_sampler_entry(lib, device):
    """The C entry point: no noise at t = 0; t = -1 and t = T (flagged in bad_t, those samples left as they are, the remaining one
    correct); refusals."""
    from dgs_amd import sampler
    d = sampler.create_diffusion("30", device=device, lib=lib)
    T = d.num_timesteps
    data = sampler_data()
    model, x_t, noise = data["render"].to(device), data["x_t"].to(device), data["noise"].to(device)
    n = SAMPLER_B * SAMPLER_PER
    # every t = 0, noise absent
    out, pred, bad = Guarded(n, device), Guarded(n, device), Guarded(1, device, dtype=torch.int32, init=torch.zeros(1, dtype=torch.int32))
    t = torch.zeros(SAMPLER_B, dtype=torch.int64, device=device)
    assert sampler_call(lib, device, d, model, x_t, None, t, True, out.t, pred.t, bad.t) == 0
    want, want_x0 = sampler_expected(d, data, [0] * SAMPLER_B, True, with_noise=False)
    assert _all_intact(out, pred, bad) and int(bad.t[0]) == 0
    assert torch.equal(out.t.view(want.shape).cpu(), want) and torch.equal(pred.t.view(want.shape).cpu(), want_x0)
    # t out of range on either side
    out, bad = Guarded(n, device), Guarded(1, device, dtype=torch.int32, init=torch.zeros(1, dtype=torch.int32))
    ts = [-1, 7, T]
    t = torch.tensor(ts, dtype=torch.int64, device=device)
    assert sampler_call(lib, device, d, model, x_t, noise, t, False, out.t, None, bad.t) == 0
    want, _ = sampler_expected(d, data, [0, 7, 0], False)
    got = out.t.view(want.shape).cpu()
    assert _all_intact(out, bad) and int(bad.t[0]) == 1
    assert bool((got[0] == FILL).all()) and bool((got[2] == FILL).all()), "a sample with t out of range was written"
    assert torch.equal(got[1], want[1])
    # refusals: nothing is written
    out, bad = Guarded(64, device), Guarded(1, device, dtype=torch.int32, init=torch.zeros(1, dtype=torch.int32))
    t = torch.tensor([7], dtype=torch.int64, device=device)
    ok = dict(per=8, offset=8, stride=16, B=1)
    small = lambda **kw: sampler_call(lib, device, d, kw.pop("model", model), kw.pop("x_t", x_t), noise, kw.pop("t", t), True, kw.pop("out", out.t), None,
                                      bad.t, **dict(ok, **kw))
    assert small(per=6) != 0 and small(offset=2) != 0 and small(stride=18) != 0 and small(per=0) != 0 and small(B=0) != 0
    assert small(model=None) != 0 and small(x_t=None) != 0 and small(t=None) != 0 and small(out=None) != 0
    assert _lib(lib).dgs_sampler_step(None, _stream(device)) != 0
    assert out.untouched() and int(bad.t[0]) == 0 and bad.intact()
    assert small() == 0                                     # the same call with valid arguments goes through
    assert bool((out.t[:8] != FILL).all()) and bool((out.t[8:] == FILL).all()) and out.intact()
