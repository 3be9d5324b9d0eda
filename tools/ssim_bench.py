"""Fused image loss (losses.image_losses: MSE + SSIM, csrc/ssim.hip) against the same loss written with torch ops (grouped F.conv2d,
autograd), forward + backward, on the same tensors, at the two training shapes (b = 4, v = 10 at 256^2; b = 4, v = 11 at 512^2).
Device events after warm-up; the two forms alternate inside one call, five pairs, every pair reported.  Kernel bytes from shapes over the
time as a share of the measured copy bandwidth (6.29 TB/s, float4 copy on the MI355X).  Writes profiles/ssim_bench.json.
    python tools/ssim_bench.py [--pairs 5] [--iters 20] [--train-step] [--out profiles/ssim_bench.json]
--train-step adds the full-size training step (24 blocks, b = 4, 4 input + 10 rendered views at 256^2) with lambda_ssim None vs 0.2.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
import torch
import torch.nn.functional as F

from dgs_amd import losses

COPY_BW = 6.29e12
LAMBDA_MSE, LAMBDA_SSIM = 1.0, 0.2
# launches per forward + backward.  fused: dgs_ssim (tile kernel + finishing kernel) + dgs_ssim_backward, and the small torch ops on
# [b] / [N] vectors around them.  torch form: 10 grouped conv2d forward (five maps, two passes each) and autograd's backward of them
# (only x needs a gradient), plus the elementwise expression and its backward: counted by the profiler run, not here.
FUSED_KERNELS = {"ssim_forward_kernel": 1, "ssim_final_kernel": 1, "ssim_backward_kernel": 1}


def window(dev):
    k = torch.arange(11, dtype=torch.float32, device=dev) - 5.0
    w = torch.exp(-(k ** 2) / (2 * 1.5 ** 2))
    return w / w.sum()


def torch_form(x, y, w):
    b, v, C = x.shape[:3]
    xs, ys = x.flatten(0, 1), y.flatten(0, 1)
    wh, ww = w.reshape(1, 1, 11, 1).repeat(C, 1, 1, 1), w.reshape(1, 1, 1, 11).repeat(C, 1, 1, 1)
    G = lambda t: F.conv2d(F.conv2d(t, wh, groups=C), ww, groups=C)
    mu1, mu2 = G(xs), G(ys)
    s1, s2, s12 = G(xs * xs) - mu1 * mu1, G(ys * ys) - mu2 * mu2, G(xs * ys) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * ((2 * s12 + C2) / (s1 + s2 + C2))
    sl = (1.0 - m.flatten(2).mean(-1).mean(-1)).reshape(b, v).mean(dim=1)
    l2 = ((x - y) ** 2).mean(dim=(1, 2, 3, 4))
    return LAMBDA_MSE * l2.mean() + LAMBDA_SSIM * sl.mean()


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3            # microseconds per forward + backward


def bench_shape(b, v, res, pairs, iters, dev):
    g = torch.Generator(device=dev).manual_seed(res)
    y = torch.rand(b, v, 3, res, res, device=dev, generator=g)
    x = (y + 0.05 * torch.randn(b, v, 3, res, res, device=dev, generator=g)).requires_grad_(True)
    w = window(dev)

    def fused():
        x.grad = None
        losses.image_losses(x, y, LAMBDA_MSE, LAMBDA_SSIM)[0].backward()

    def library():
        x.grad = None
        torch_form(x, y, w).backward()

    fused()
    ga = x.grad.clone()
    library()
    agree = float((ga - x.grad).abs().max() / x.grad.abs().max())
    for _ in range(3):
        fused()
        library()
    torch.cuda.synchronize()
    rows = []
    for _ in range(pairs):
        rows.append((timed(fused, iters), timed(library, iters)))
    P = 4.0 * b * v * 3 * res * res                       # one f32 image tensor
    maps = 3 * 4.0 * b * v * 3 * (res - 10) ** 2          # the three saved maps
    nbytes = (2 * P + maps) + (maps + 2 * P + P)          # forward: x, y in, maps out; backward: maps, x, y in, dx out
    fa, fb = [r[0] for r in rows], [r[1] for r in rows]
    best = min(fa)
    out = dict(shape=[b, v, 3, res, res], pairs_us=[dict(fused=round(a, 1), torch_ops=round(t, 1)) for a, t in rows],
               fused_us=dict(min=round(min(fa), 1), max=round(max(fa), 1)), torch_ops_us=dict(min=round(min(fb), 1), max=round(max(fb), 1)),
               fused_faster_in_every_pair=all(a < t for a, t in rows), speedup_min=round(min(t / a for a, t in rows), 2),
               kernel_bytes=int(nbytes), share_of_copy_bandwidth=round(nbytes / (best * 1e-6) / COPY_BW, 3),
               gradient_max_deviation_between_forms=agree)
    print(json.dumps(out), flush=True)
    return out


def train_step(lambda_ssim, steps, dev):
    import numpy as np
    from dgs_amd import cameras, denoiser as dn, synth
    from dgs_amd.optim import FusedAdamW
    from dgs_amd.train import DataParallelTrainer
    B, res, V, RV = 4, 256, 4, 10
    batch, t = synth.make_batch(B, res, V=V, device=dev, seed=100, with_t=True)
    extra = torch.tensor(np.stack([cameras.ring_cameras(RV - V, phase_deg=5.0 + 7 * b) for b in range(B)])).to(dev)
    rc2w = torch.cat([batch["c2w"], extra.to(batch["c2w"].dtype)], 1).contiguous()
    rk = torch.tensor(cameras.default_fxfycxcy(res)).expand(B, RV, 4).contiguous().to(dev)
    target = torch.rand(B, RV, 3, res, res, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    m = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=24, ray_pe_type="relative_plk"), device=dev)
    m.reset_parameters(seed=0)
    m = m.to(dev)
    m.train()
    with DataParallelTrainer(m, FusedAdamW(m, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.05), max_grad_norm=0.5, lambda_ssim=lambda_ssim) as tr:
        for _ in range(3):
            tr.step(batch, t, target, rc2w, rk)
        torch.cuda.synchronize()
        ms = timed(lambda: tr.step(batch, t, target, rc2w, rk), steps) / 1e3
    del m
    torch.cuda.empty_cache()
    return round(ms, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ssim_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), lambda_mse=LAMBDA_MSE, lambda_ssim=LAMBDA_SSIM, copy_bandwidth=COPY_BW,
               fused_kernel_launches=FUSED_KERNELS, shapes=[bench_shape(4, 10, 256, a.pairs, a.iters, dev), bench_shape(4, 11, 512, a.pairs, a.iters, dev)])
    if a.train_step:
        res["train_step_ms"] = {"lambda_ssim=None": train_step(None, 10, dev), "lambda_ssim=0.2": train_step(0.2, 10, dev)}
        print(json.dumps(res["train_step_ms"]), flush=True)
    res["done"] = all(s["fused_faster_in_every_pair"] for s in res["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out, "| fused faster in every pair at both shapes:", res["done"])
    sys.exit(0 if res["done"] else 1)


if __name__ == "__main__":
    main()
