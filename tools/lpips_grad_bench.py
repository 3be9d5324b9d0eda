"""The differentiable LPIPS call (dgs_amd.lpips.LPIPS(differentiable=True): dgs_lpips_forward_backward, csrc/lpips.hip) against the same
network written with torch ops and torch autograd (F.conv2d = MIOpen) on the same device, the forward against the parent commit's
library, and the parity ratios of tests/lpips_grad_util.py.  Seeded random weights (the library ships none).
    python tools/lpips_grad_bench.py [--pairs 5]                  16 and 40 pairs of 256^2, gradient to x0 only: the whole call plus
                                                                  .backward() (ours: allocation, forward, backward sequence, the stored
                                                                  gradient times grad_out), alternating with torch inside one process
    python tools/lpips_grad_bench.py --only-ours N [--batch 16]   N such calls of ours and nothing else (the target of a rocprofv3
                                                                  --kernel-trace --stats run)
    python tools/lpips_grad_bench.py --kernel-stats TXT --batch 16 --calls N       no GPU: adds each kernel's time per call from TXT
    python tools/lpips_grad_bench.py --forward-side N             one process: N forward calls under no_grad, 16 pairs; prints a JSON line
    python tools/lpips_grad_bench.py --forward-ab BASE.so         three alternating pairs of processes (BASE.so = the parent commit's
                                                                  library, tools/ab_build.sh lpips.hip <rev>; this tree's library) and
                                                                  three pairs of this tree's library against itself (the A/A spread)
    python tools/lpips_grad_bench.py --train-step                 informative: DataParallelTrainer.train_step with lambda_lpips = 0.5 through
                                                                  the module and through the torch-op form, at the configuration of
                                                                  tools/train_objective_bench.py (b = 4, 4 + 10 views at 256^2: 40 pairs)
    python tools/lpips_grad_bench.py --parity DEVICE --parity-out FILE             appends the measured / bar ratios for cpu or cuda:0
Writes profiles/lpips_grad_bench.json.  Needs a GPU except for --kernel-stats and --parity cpu: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = (16, 40)
RES = 256
KERNELS = ("conv3x3_kernel", "maxpool2x2_kernel", "maxpool2x2_backward_kernel", "lpips_input_kernel", "lpips_input_backward_kernel",
           "lpips_tap_pixel_kernel", "lpips_tap_mean_kernel", "lpips_tap_backward_kernel", "lpips_finish_kernel")


PEAK_F32_MATRIX = 157.3e12


def conv_flops(images, res=RES, backward=False):
    """2 * 9 * Cin * Cout * H * W summed over the thirteen convolutions, from shapes (backward: the thirteen data gradients, the first
    one at its shape 64 -> 3, not at the 64 -> 64 it is padded to)."""
    from dgs_amd import lpips as P
    total, h, w = 0, res, res
    for i, (cin, cout) in enumerate(P.CONV_CHANNELS):
        if i in P.POOL_BEFORE:
            h, w = h // 2, w // 2
        total += 2 * 9 * cin * cout * h * w
    return total * images


def add_kernel_stats(args):
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rows = {}
    for line in open(args.kernel_stats):
        for name in KERNELS:
            if name + "(" in line.replace("<", "(") and line.lstrip().startswith(("dgs::", "void dgs::")):
                calls, total_us = line.split()[-6:-4]                         # ... calls total_us avg_us min_us max_us pct
                grad = "conv3x3_kernel" in name and line.split("conv3x3_kernel<")[1].split(">")[0].replace(" ", "").endswith("true")
                r = rows.setdefault(name + (" (data gradient)" if grad else ""), {"launches": 0, "us_per_call": 0.0})
                r["launches"] += int(calls)
                r["us_per_call"] += float(total_us) / args.calls
    s = out.setdefault(f"{args.batch}_pairs", {})
    s["kernels"] = rows
    fwd, bwd = rows.get("conv3x3_kernel"), rows.get("conv3x3_kernel (data gradient)")
    if fwd and bwd:
        s["forward_conv_share_of_f32_matrix_peak"] = conv_flops(2 * args.batch) / (fwd["us_per_call"] * 1e-6) / PEAK_F32_MATRIX
        s["data_gradient_share_of_f32_matrix_peak"] = conv_flops(args.batch, backward=True) / (bwd["us_per_call"] * 1e-6) / PEAK_F32_MATRIX
        s["data_gradient_over_forward_conv_time"] = bwd["us_per_call"] / fwd["us_per_call"]
    s["kernels_source"] = os.path.relpath(args.kernel_stats, ROOT) + f" (rocprofv3 --kernel-trace --stats, a run of its own, {args.calls} calls, the warm-up among them)"
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def parity(args):
    import lpips_grad_util as GU
    emu = args.parity == "cpu"
    what = "CPU emulation build of the kernels" if emu else "MI355X, product library"
    lines = [f"# {what}: measured error / bar (<= 1 passes); bars as stated in tests/lpips_grad_util.py",
             "# tap backward against fp64 autograd, bar 8 x the relative L2 error of fp32 torch autograd on the CPU"]
    for c in GU.TAP_CASES:
        r = GU.check_tap_backward(args.parity, *c)
        lines.append(f"tap backward  N={c[0]} H={c[1]} W={c[2]} C={c[3]:<4d} worst {max(x[1] for x in r):.4f}   (x the fp32 autograd's error: {8 * max(x[1] for x in r):.2f})")
    lines.append("# whole network, d out.sum() / d image against fp64 autograd of the restatement, bar 8 x the fp32 restatement's relative L2 error")
    cases = [(2, 16, 16)] if emu else GU.NET_CASES
    worst = 0.0
    for c in cases:
        for name, ratio, e, e32 in GU.check_network_grad(args.parity, *c):
            worst = max(worst, ratio)
            lines.append(f"network  n={c[0]} {c[1]}x{c[2]:<3d} {name:<18s} {ratio:.4f}   rel-L2 {e:.3e}, fp32 restatement {e32:.3e} ({e / e32:.2f} x)")
    lines.append(f"# {len(cases)} network cases, largest ratio {worst:.4f} ({8 * worst:.2f} x the fp32 restatement's error)")
    with open(args.parity_out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
    print("\n".join(lines))


def forward_side(args):
    import torch

    import lpips_util as LU
    dev = torch.device("cuda:0")
    model = LU.model(dev)
    x0, x1 = (t.to(dev) for t in LU.images(16, RES, RES, seed=16))
    times = []
    with torch.no_grad():
        for i in range(args.forward_side + 3):
            torch.cuda.synchronize()
            t0 = time.time()
            model(x0, x1)
            torch.cuda.synchronize()
            if i >= 3:
                times.append(time.time() - t0)
    print(json.dumps({"median_s": statistics.median(times), "min_s": min(times), "calls": len(times)}))


def forward_ab(args):
    def side(library):
        env = dict(os.environ)
        env.pop("DGS_AMD_LIBRARY", None)
        if library:
            env["DGS_AMD_LIBRARY"] = os.path.abspath(library)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-side", "20"], env=env, stdout=subprocess.PIPE, text=True, timeout=300,
                           check=True)
        return json.loads(r.stdout.strip().splitlines()[-1])["median_s"]

    ab, aa = [], []
    for _ in range(3):
        base, new = side(args.forward_ab), side(None)
        ab.append({"parent_s": base, "this_s": new, "this_over_parent": new / base})
        first, second = side(None), side(None)
        aa.append({"first_s": first, "second_s": second, "second_over_first": second / first})
        print(ab[-1], aa[-1], flush=True)
    spread = max(abs(r["second_over_first"] - 1) for r in aa)
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["forward_against_parent"] = {
        "what": "LPIPS.forward under no_grad, 16 pairs of 256^2, median wall seconds of 20 calls per process; three alternating pairs of "
                "processes parent / this tree, and three pairs this tree / this tree (A/A)",
        "parent_library": "tools/ab_build.sh lpips.hip <parent revision>", "pairs": ab, "a_a_pairs": aa, "a_a_spread": spread,
        "mean_this_over_parent": statistics.mean(r["this_over_parent"] for r in ab),
        "inside_a_a_spread": abs(statistics.mean(r["this_over_parent"] for r in ab) - 1) <= spread}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out["forward_against_parent"])


def train_step(args):
    import numpy as np
    import torch

    import lpips_grad_util as GU
    import lpips_util as LU
    from dgs_amd import cameras, denoiser as dn, sampler
    from dgs_amd.optim import FusedAdamW
    from dgs_amd.train import DataParallelTrainer
    dev = torch.device("cuda:0")
    B, res, V, RV = 4, 256, 4, 10                                             # tools/train_objective_bench.py's batch
    g = torch.Generator(device=dev).manual_seed(1)
    c2w = torch.tensor(np.stack([cameras.ring_cameras(RV, phase_deg=5.0 + 7 * b) for b in range(B)]), dtype=torch.float32).to(dev)
    k = torch.tensor(cameras.default_fxfycxcy(res), dtype=torch.float32).expand(B, RV, 4).contiguous().to(dev)
    rgbs = torch.rand(B, RV, 3, res, res, device=dev, generator=g)
    batch = {"rgbs_input": rgbs[:, :V].contiguous(), "c2ws_input": c2w[:, :V].contiguous(), "fxfycxcys_input": k[:, :V].contiguous(),
             "depths_input": 1.5 + torch.rand(B, V, 1, res, res, device=dev, generator=g), "masks_input": torch.ones(B, V, 1, res, res, device=dev),
             "c2ws": c2w, "fxfycxcys": k, "rgbs": rgbs, "masks": torch.ones(B, RV, 1, res, res, device=dev)}
    d = sampler.create_diffusion("1000", device=dev)
    m = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=args.layers, ray_pe_type="relative_plk"), device=dev)
    m.reset_parameters(seed=0)
    m = m.to(dev).train()
    module = GU.grad_model(dev)
    sd = {k_: v.to(dev) for k_, v in LU.random_state_dict(0).items()}
    torch_form = lambda x, y: LU.restatement_impl(sd, x, y, torch.float32, lambda t: t)[0]
    loss = dict(lambda_diffusion=1.0, lambda_lpips=0.5)

    def timed(fn, steps=3):
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.time() - t0) / steps

    rows = []
    with DataParallelTrainer(m, FusedAdamW(m, lr=1e-5, betas=(0.9, 0.99), weight_decay=0.05), max_grad_norm=0.5) as tr:
        def side(perceptual):
            tr.configure_objective(d, loss, perceptual=perceptual)
            tr.train_step(batch)                                              # the first step after a change of the objective is not timed
            return timed(lambda: tr.train_step(batch))
        side(module), side(torch_form)
        for _ in range(3):
            rows.append({"module_s": side(module), "torch_ops_s": side(torch_form)})
            rows[-1]["torch_ops_over_module"] = rows[-1]["torch_ops_s"] / rows[-1]["module_s"]
            print(rows[-1], flush=True)
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["train_step"] = {"what": "informative: wall seconds per DataParallelTrainer.train_step (mean of 3), lambda_diffusion = 1, lambda_lpips = 0.5, the "
                                 "perceptual term over 40 pairs of 256^2; three alternating pairs inside one process",
                         "configuration": dict(b=B, input_views=V, rendered_views=RV, res=res, layers=args.layers, width=1024),
                         "alternating_pairs": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--forward-side", type=int, default=0)
    ap.add_argument("--forward-ab", default=None)
    ap.add_argument("--parity", default=None)
    ap.add_argument("--parity-out", default=os.path.join(ROOT, "profiles", "lpips_grad_parity.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_grad_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args)
    if args.parity:
        return parity(args)
    if args.forward_side:
        return forward_side(args)
    if args.forward_ab:
        return forward_ab(args)
    if args.train_step:
        return train_step(args)

    import torch

    import lpips_grad_util as GU
    import lpips_util as LU

    dev = torch.device("cuda:0")
    model = GU.grad_model(dev)
    sd = {k: v.to(dev) for k, v in LU.random_state_dict(0).items()}

    def ours(x0, x1):
        a = x0.clone().requires_grad_(True)
        model(a, x1).sum().backward()
        return a.grad

    def torch_ops(x0, x1):
        a = x0.clone().requires_grad_(True)
        LU.restatement_impl(sd, a, x1, torch.float32, lambda t: t)[0].sum().backward()
        return a.grad

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return out, time.time() - t0

    if args.only_ours:
        x0, x1 = (t.to(dev) for t in LU.images(args.batch, RES, RES, seed=1))
        for _ in range(args.only_ours):
            ours(x0, x1)
        torch.cuda.synchronize()
        return
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out.update({"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each", "resolution": RES,
                "ours": "LPIPS(differentiable=True)(x0, x1).sum().backward(), x0 requiring grad: allocation, dgs_lpips_forward_backward (forward "
                        "keeping 13 ReLU outputs; 5 tap gradients, 13 data gradients over the x0 images, 4 pool gradients), stored gradient x grad_out",
                "comparator": "the same network with torch ops in fp32 on the device and torch autograd (F.conv2d = MIOpen): "
                              "tests/lpips_util.py restatement_impl, .sum().backward()"})
    for n in BATCHES:
        x0, x1 = (t.to(dev) for t in LU.images(n, RES, RES, seed=n))
        ours(x0, x1)
        torch_ops(x0, x1)                                                     # warm-up of both (MIOpen's find step among it)
        torch.cuda.reset_peak_memory_stats()
        ours(x0, x1)
        peak_ours = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        torch_ops(x0, x1)
        peak_torch = torch.cuda.max_memory_allocated()
        rows = []
        for _ in range(args.pairs):
            g, t_o = timed(lambda: ours(x0, x1))
            h, t_t = timed(lambda: torch_ops(x0, x1))
            rows.append({"ours_s": t_o, "torch_s": t_t, "torch_over_ours": t_t / t_o})
            print(n, rows[-1], flush=True)
        s = out.setdefault(f"{n}_pairs", {})
        if n == BATCHES[0]:                                                   # both fp32 forms against fp64 autograd of the restatement, 4 pairs at a time
            sd64 = {k: v.double() for k, v in sd.items()}
            g64 = []
            for i in range(0, n, 4):
                a = x0[i:i + 4].double().requires_grad_(True)
                LU.restatement_impl(sd64, a, x1[i:i + 4].double(), torch.float64, lambda t: t)[0].sum().backward()
                g64.append(a.grad)
            g64 = torch.cat(g64)
            s["relative_l2_to_fp64_autograd"] = {"ours": float((g.double() - g64).norm() / g64.norm()), "torch_fp32": float((h.double() - g64).norm() / g64.norm())}
        s.update({"alternating_pairs": rows, "faster_than_torch_in_every_pair": all(r["torch_over_ours"] > 1 for r in rows),
                  "slower_than_torch_in_every_pair": all(r["torch_over_ours"] < 1 for r in rows),
                  "relative_l2_to_torch": float((g - h).norm() / h.norm()),
                  "peak_allocated_bytes_ours": int(peak_ours), "peak_allocated_bytes_torch": int(peak_torch),
                  "ours_same_bytes_in_two_calls": bool(torch.equal(g, ours(x0, x1))),
                  "torch_same_bytes_in_two_calls": bool(torch.equal(h, torch_ops(x0, x1)))})
        print(n, {k: v for k, v in s.items() if k != "alternating_pairs"}, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
