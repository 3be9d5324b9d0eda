"""The LPIPS-VGG forward on the device (dgs_amd.lpips.LPIPS.forward -> dgs_lpips_forward, csrc/lpips.hip) against the same network
written with torch ops (F.conv2d in fp32, F.max_pool2d, the tap formulas) on the same device, which runs MIOpen's convolutions.
    16 pairs of 256^2    eval_scene_result.py's chunk of 8 files, both images of a pair
    40 pairs of 256^2    the training step's b * v
Seeded random weights (the library ships none).  --pairs alternating pairs (ours, torch) per batch inside one process; wall time around
a device synchronisation; `ours` is the whole call: workspace allocation, the input kernel, 13 convolutions, 4 pools, 5 taps.
Writes profiles/lpips_bench.json.
    python tools/lpips_bench.py [--pairs 5] [--out profiles/lpips_bench.json]
    python tools/lpips_bench.py --only-ours N [--batch 16]        N calls of ours and nothing else (the target of a rocprofv3
                                                                  --kernel-trace --stats run)
    python tools/lpips_bench.py --kernel-stats TXT --batch 16 --calls N --out FILE    no GPU: adds to FILE each kernel's time in TXT per
                                                                  forward call and the convolutions' share of the fp32-matrix peak
Needs a GPU except for --kernel-stats: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F32_MATRIX = 157.3e12
BATCHES = (16, 40)
RES = 256
KERNELS = ("conv3x3_kernel", "maxpool2x2_kernel", "lpips_input_kernel", "lpips_tap_pixel_kernel", "lpips_tap_mean_kernel", "lpips_finish_kernel")


def conv_flops(images, res=RES):
    """2 * 9 * Cin * Cout * H * W summed over the thirteen convolutions, from shapes."""
    from dgs_amd import lpips as P
    total, h, w = 0, res, res
    for i, (cin, cout) in enumerate(P.CONV_CHANNELS):
        if i in P.POOL_BEFORE:
            h, w = h // 2, w // 2
        total += 2 * 9 * cin * cout * h * w
    return total * images


def add_kernel_stats(args):
    out = json.load(open(args.out))
    rows = {}
    for line in open(args.kernel_stats):
        for name in KERNELS:
            if name in line and line.lstrip().startswith(("dgs::", "void dgs::")):
                calls, total_us, avg_us = line.split()[-6:-3]                  # ... calls total_us avg_us min_us max_us pct
                r = rows.setdefault(name, {"launches": 0, "us_per_forward_call": 0.0})
                r["launches"] += int(calls)
                r["us_per_forward_call"] += float(total_us) / args.calls
    s = out.setdefault(f"{args.batch}_pairs", {})
    s["kernels"] = rows
    s["kernels_source"] = os.path.relpath(args.kernel_stats, ROOT) + f" (rocprofv3 --kernel-trace --stats, a run of its own, {args.calls} forward calls, the warm-up among them)"
    if "conv3x3_kernel" in rows:
        flops = conv_flops(2 * args.batch)
        s["conv_flops_from_shapes"] = flops
        s["conv_share_of_f32_matrix_peak"] = flops / (rows["conv3x3_kernel"]["us_per_forward_call"] * 1e-6) / PEAK_F32_MATRIX
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args)

    import torch

    import lpips_util as LU

    dev = torch.device("cuda:0")
    model = LU.model(dev)
    sd = {k: v.to(dev) for k, v in LU.random_state_dict(0).items()}

    def torch_lpips(x0, x1):
        with torch.no_grad():
            return LU.restatement_on(sd, x0, x1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return out, time.time() - t0

    if args.only_ours:
        x0, x1 = (t.to(dev) for t in LU.images(args.batch, RES, RES, seed=1))
        for _ in range(args.only_ours):
            model(x0, x1)
        torch.cuda.synchronize()
        return
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out.update({"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each", "resolution": RES,
                "ours": "dgs_amd.lpips.LPIPS.forward: allocation, dgs_lpips_forward (input kernel, 13 convolutions on the f32 MFMA, 4 pools, 5 taps)",
                "comparator": "the same network with torch ops in fp32 on the device (F.conv2d = MIOpen, F.max_pool2d, the tap formulas): "
                              "tests/lpips_util.py restatement_on",
                "f32_matrix_peak_flops": PEAK_F32_MATRIX})
    for n in BATCHES:
        x0, x1 = (t.to(dev) for t in LU.images(n, RES, RES, seed=n))
        model(x0, x1)
        torch_lpips(x0, x1)                                                   # warm-up of both (MIOpen's find step among it)
        rows = []
        for _ in range(args.pairs):
            ours, t_o = timed(lambda: model(x0, x1))
            theirs, t_t = timed(lambda: torch_lpips(x0, x1))
            rows.append({"ours_s": t_o, "torch_s": t_t, "torch_over_ours": t_t / t_o})
            print(n, rows[-1], flush=True)
        flops = conv_flops(2 * n)
        best = min(r["ours_s"] for r in rows)
        s = out.setdefault(f"{n}_pairs", {})
        s.update({"alternating_pairs": rows, "conv_flops_from_shapes": flops, "whole_call_share_of_f32_matrix_peak_best": flops / best / PEAK_F32_MATRIX,
                  "faster_than_torch_in_every_pair": all(r["torch_over_ours"] > 1 for r in rows),
                  "largest_relative_difference_to_torch": float(((ours.reshape(-1) - theirs) / theirs).abs().max()),
                  "ours_same_bytes_in_two_calls": bool(torch.equal(ours, model(x0, x1))),
                  "torch_same_bytes_in_two_calls": bool(torch.equal(theirs, torch_lpips(x0, x1)))})
        print(n, {k: v for k, v in s.items() if k != "alternating_pairs"}, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
