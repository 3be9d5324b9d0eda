"""DataParallelTrainer.train_step (the reference's objective from a CLEAN batch: draws, HIP rays, one dgs_train_inputs launch, then the
loop of step()) against DataParallelTrainer.step on inputs that were noised beforehand with torch ops, at the bench's training
configuration (24 blocks, width 1024, b = 4, 4 input + 10 rendered views at 256^2, FusedAdamW, clip 0.5).  Both sides train on
lambda_diffusion alone.  One model, one trainer, the two calls alternate inside one process; every pair is reported.
Also: dgs_train_inputs alone at that shape (with the xyz target) against the bytes it must move, computed from the shapes, as a share of
the measured copy bandwidth (6.29 TB/s, float4 copy on the MI355X; the 77 MB it touches fit the Infinity Cache, so a share above 1 is
possible and says so).  Writes profiles/train_objective_bench.json.
    python tools/train_objective_bench.py [--pairs 5] [--steps 5] [--layers 24] [--out profiles/train_objective_bench.json]
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
import numpy as np
import torch

COPY_BW = 6.29e12


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters            # milliseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_objective_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/train_objective_bench.py needs a GPU")
    from dgs_amd import cameras, denoiser as dn, sampler
    from dgs_amd.optim import FusedAdamW
    from dgs_amd.train import DataParallelTrainer
    dev = torch.device("cuda:0")
    B, res, V, RV = 4, 256, 4, 10
    g = torch.Generator(device=dev).manual_seed(1)
    c2w = torch.tensor(np.stack([cameras.ring_cameras(RV, phase_deg=5.0 + 7 * b) for b in range(B)]), dtype=torch.float32).to(dev)
    k = torch.tensor(cameras.default_fxfycxcy(res), dtype=torch.float32).expand(B, RV, 4).contiguous().to(dev)
    rgbs = torch.rand(B, RV, 3, res, res, device=dev, generator=g)
    batch = {"rgbs_input": rgbs[:, :V].contiguous(), "c2ws_input": c2w[:, :V].contiguous(), "fxfycxcys_input": k[:, :V].contiguous(),
             "depths_input": 1.5 + torch.rand(B, V, 1, res, res, device=dev, generator=g), "masks_input": torch.ones(B, V, 1, res, res, device=dev),
             "c2ws": c2w, "fxfycxcys": k, "rgbs": rgbs, "masks": torch.ones(B, RV, 1, res, res, device=dev)}
    d = sampler.create_diffusion("1000", device=dev)
    m = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=a.layers, ray_pe_type="relative_plk"), device=dev)
    m.reset_parameters(seed=0)
    m = m.to(dev).train()
    # the other side's inputs, noised beforehand with torch ops (outside the timed region)
    noise = torch.randn(B, V, 3, res, res, device=dev, generator=g)
    t = torch.randint(0, 1000, (B,), device=dev, generator=g)
    ca, cs = d._sqrt_acp[t].reshape(B, 1, 1, 1, 1), d._sqrt_1m_acp[t].reshape(B, 1, 1, 1, 1)
    x_t = batch["rgbs_input"].clone()
    x_t[:, 1:] = ca * x_t[:, 1:] + cs * noise[:, 1:]
    ray_o, ray_d = m.gs_renderer.backend().rays_from_c2w(batch["c2ws_input"], batch["fxfycxcys_input"], res, res)
    pre = dict(image=x_t, ray_o=ray_o, ray_d=ray_d, c2w=c2w, fxfycxcy=k)
    rows = []
    with DataParallelTrainer(m, FusedAdamW(m, lr=1e-5, betas=(0.9, 0.99), weight_decay=0.05), max_grad_norm=0.5) as tr:
        tr.configure_objective(d, dict(lambda_diffusion=1.0))
        objective = lambda: tr.train_step(batch)
        plain = lambda: tr.step(pre, t, rgbs)
        for _ in range(3):
            objective()
            plain()
        torch.cuda.synchronize()
        for _ in range(a.pairs):
            rows.append((timed(objective, a.steps), timed(plain, a.steps)))
            print(json.dumps(dict(train_step_ms=round(rows[-1][0], 3), step_ms=round(rows[-1][1], 3))), flush=True)
        assert int(d.bad_t[0]) == 0
    # the launch alone, with the xyz target
    call = lambda: d.training_inputs(batch["rgbs_input"], t, noise, batch["depths_input"], ray_o, ray_d)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    kernel_us = [timed(call, 50) * 1e3 for _ in range(a.pairs)]          # includes the two output allocations of the wrapper (cached blocks)
    P = 4.0 * B * V * 3 * res * res
    nbytes = P + P * (V - 1) / V + P / 3 + 2 * P + 2 * P                  # image, noise of the noisy views, depth, ray_o, ray_d in; x_t, xyz out
    diffs = [o - p for o, p in rows]
    out = dict(device=torch.cuda.get_device_name(0), configuration=dict(b=B, input_views=V, rendered_views=RV, res=res, layers=a.layers, width=1024),
               steps_per_timing=a.steps, pairs_ms=[dict(train_step=round(o, 3), step=round(p, 3)) for o, p in rows],
               train_step_ms=dict(min=round(min(o for o, _ in rows), 3), max=round(max(o for o, _ in rows), 3)),
               step_ms=dict(min=round(min(p for _, p in rows), 3), max=round(max(p for _, p in rows), 3)),
               train_step_minus_step_ms=dict(min=round(min(diffs), 3), max=round(max(diffs), 3)),
               train_inputs=dict(shape=[B, V, 3, res, res], with_xyz_target=True, call_us=[round(x, 2) for x in kernel_us], bytes=int(nbytes),
                                 copy_bandwidth=COPY_BW, bytes_over_copy_bandwidth_us=round(nbytes / COPY_BW * 1e6, 2),
                                 share_of_copy_bandwidth=round(nbytes / (min(kernel_us) * 1e-6) / COPY_BW, 3)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["train_inputs"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
