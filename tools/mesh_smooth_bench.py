"""The mesh smoothing on the device (consumers.smooth_mesh -> dgs_mesh_smooth, csrc/mesh_smooth.hip) against the same smoothing written
with torch ops on the same device: per call the neighbour pairs of the faces and the incidence counts (index_add_ of ones), per pass
one index_add_ of the fp32 neighbour positions, a division and the step.  Its fp32 atomics give different bytes from run to run; it is
what a user without this call would write.
    R = 256, nb = 64, N = 262,144    the pipeline's setting: the mesh after the component filters (about 1.57 M faces) and that mesh
                                     decimated to the reference's 1e5 faces (about 99 k)
Both at the defaults (10 iterations, 0.5, -0.53).  --pairs alternating pairs (ours, torch) per mesh inside one process; wall time around
a device synchronisation; `ours` is the whole call: workspace and output allocation, the build of the incidence list, 20 passes.
Writes profiles/mesh_smooth_bench.json.
    python tools/mesh_smooth_bench.py [--pairs 5] [--out profiles/mesh_smooth_bench.json]
    python tools/mesh_smooth_bench.py --only-ours N [--mesh NAME]    N calls of ours and nothing else (the target of a rocprofv3
                                                                     --kernel-trace --stats run)
    python tools/mesh_smooth_bench.py --extract-only LABEL --out FILE   extract_mesh() with its default arguments at R = 256 and R = 128,
                                                                     --pairs calls twice over (an A/A pair of medians), appended to
                                                                     FILE under LABEL: run once with this tree's library and once with
                                                                     DGS_AMD_LIBRARY = the parent's
    python tools/mesh_smooth_bench.py --kernel-stats TXT --mesh NAME --calls N --out FILE   no GPU: adds to FILE each kernel's time in TXT
                                                                     per smooth_mesh call, the build against the passes, and the
                                                                     passes' bytes from shapes against the copy bandwidth
    python tools/mesh_smooth_bench.py --ab-summary --out FILE        no GPU: the ratio of the medians (this / parent) of the
                                                                     --extract-only rows in FILE next to the A/A spread
Needs a GPU except for --kernel-stats and --ab-summary: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_BW = 6.29e12
LEVEL, MIN_F, MIN_D, TARGET = 0.005, 64, 20, 1e5
ITERATIONS, LAM, MU = 10, 0.5, -0.53
SETTINGS = (("r128_nb32_n65536", 65536, 31, 128, 32), ("r256_nb64_n262144", 262144, 21, 256, 64))
MESHES = ("decimated", "undecimated")
BUILD = ("sm_count_kernel", "sm_scan_kernel", "sm_sums_kernel", "sm_fill_kernel")
KERNELS = BUILD + ("sm_pass_kernel",)


def pass_bytes(V, F):
    """Bytes one sm_pass_kernel launch must move at the least, from shapes: cnt, start and the vertex's own position read, the 6 F
    neighbour indices read, each gathered position counted once as 12 B (a vertex's position is gathered 2 c_v times, from the caches
    at best), the new position written."""
    return {"at_least": 4 * V + 4 * V + 12 * V + 24 * F + 12 * V, "every_gather_from_memory": 4 * V + 4 * V + 12 * V + 24 * F + 72 * F + 12 * V}


def add_kernel_stats(args):
    out = json.load(open(args.out))
    s = out[args.mesh]
    rows, mine = {}, True
    for line in open(args.kernel_stats):
        if line.startswith("#"):                                              # one section a mesh, headed by the command that made it
            mine = "--mesh " + args.mesh in line
        for name in KERNELS:
            if mine and line.startswith("dgs::" + name + "("):
                calls, total_us, avg_us = line.split()[-6:-3]                  # ... calls total_us avg_us min_us max_us pct
                rows[name] = {"launches": int(calls), "avg_us": float(avg_us), "us_per_smooth_mesh_call": float(total_us) / args.calls}
    moved = pass_bytes(s["V"], s["F"])
    p = rows["sm_pass_kernel"]
    p["bytes_from_shapes"] = moved
    p["share_of_copy_bandwidth"] = {k: b / (p["avg_us"] * 1e-6) / COPY_BW for k, b in moved.items()}
    s["kernels"] = rows
    s["kernels_source"] = os.path.relpath(args.kernel_stats, ROOT) + f" (rocprofv3 --kernel-trace --stats, a run of its own, {args.calls} smooth_mesh calls, the warm-up among them)"
    s["build_us_per_call"] = sum(rows[k]["us_per_smooth_mesh_call"] for k in BUILD if k in rows)
    s["passes_us_per_call"] = p["us_per_smooth_mesh_call"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def add_ab_summary(args):
    """Per setting: the median over all calls of each side, their ratio, and the A/A spread: the largest ratio between two medians of
    one side (every process gives two)."""
    out = json.load(open(args.out))
    summary = {}
    for name, sides in out["extract_mesh_default_arguments"].items():
        med = {k: statistics.median(t for row in rows for run in row["extract_mesh_s"] for t in run) for k, rows in sides.items()}
        halves = {k: [m for row in rows for m in row["medians_s"]] for k, rows in sides.items()}
        spread = max(max(h) / min(h) for h in halves.values())
        ratio = med["this"] / med["parent"]
        summary[name] = {"median_s": med, "this_over_parent": ratio, "a_a_spread_largest_ratio_of_two_medians_of_one_side": spread,
                         "inside_the_a_a_spread": 1 / spread <= ratio <= spread}
        print(name, summary[name])
    out["extract_mesh_default_arguments_summary"] = summary
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def torch_smooth(v, f, iterations=ITERATIONS, lam=LAM, mu=MU):
    """The comparator: valid, non-null faces assumed (the meshes here have no others); fp32 sums by index_add_."""
    import torch
    f = f.long()
    own = torch.cat((f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]))
    other = torch.cat((f[:, 1], f[:, 2], f[:, 0], f[:, 2], f[:, 0], f[:, 1]))
    cnt = torch.zeros(v.shape[0], dtype=torch.float32, device=v.device).index_add_(0, own, torch.ones(own.shape[0], dtype=torch.float32, device=v.device))
    moving = (cnt > 0)[:, None]
    cnt = cnt.clamp(min=1)[:, None]
    p = v
    for _ in range(iterations):
        for w in (lam, mu):
            m = torch.zeros_like(p).index_add_(0, own, p[other]) / cnt
            p = torch.where(moving, p + w * (m - p), p)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--mesh", default=None, choices=MESHES)
    ap.add_argument("--extract-only", default=None, metavar="LABEL")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--ab-summary", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args)
    if args.ab_summary:
        return add_ab_summary(args)

    import torch

    import field_util as U
    from dgs_amd import consumers

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return out, time.time() - t0

    dev = torch.device("cuda:0")
    if args.extract_only:
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        for name, n, seed, r, nb in SETTINGS:
            model = U.make_model(U.make_scene(n, seed), dev)
            model.extract_mesh(LEVEL, r, nb)                                  # warm-up: library load, allocator
            runs = [[timed(lambda: model.extract_mesh(LEVEL, r, nb))[1] for _ in range(args.pairs)] for _ in range(2)]
            row = {"library": os.path.basename(os.environ.get("DGS_AMD_LIBRARY", "product")), "extract_mesh_s": runs, "medians_s": [statistics.median(x) for x in runs]}
            out.setdefault("extract_mesh_default_arguments", {}).setdefault(name, {}).setdefault(args.extract_only, []).append(row)
            print(name, args.extract_only, row["medians_s"], flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    name, n, seed, r, nb = SETTINGS[1]
    model = U.make_model(U.make_scene(n, seed), dev)
    raw = model.extract_mesh(LEVEL, r, nb, min_f=MIN_F, min_d=MIN_D)
    small = consumers.decimate_mesh(raw.vertices, raw.faces, TARGET)
    meshes = {k: m for k, m in (("decimated", small), ("undecimated", (raw.vertices, raw.faces))) if args.mesh in (None, k)}
    for v, f in meshes.values():
        consumers.smooth_mesh(v, f)                                           # warm-up
    if args.only_ours:
        for _ in range(args.only_ours):
            for v, f in meshes.values():
                consumers.smooth_mesh(v, f)
        torch.cuda.synchronize()
        return
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out.update({"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each",
                "setting": name, "min_f": MIN_F, "min_d": MIN_D, "target_faces": TARGET, "iterations": ITERATIONS, "lambda": LAM, "mu": MU,
                "ours": "consumers.smooth_mesh(vertices, faces): allocation, the build of the incidence list, 20 passes",
                "comparator": "the same smoothing with torch ops on the device: neighbour pairs and counts per call, per pass one "
                              "index_add_ of fp32 positions, a division, the step (tools/mesh_smooth_bench.py torch_smooth)"})
    for key, (v, f) in meshes.items():
        torch_smooth(v, f)                                                    # warm-up
        rows = []
        for _ in range(args.pairs):
            ours, t_o = timed(lambda: consumers.smooth_mesh(v, f))
            theirs, t_t = timed(lambda: torch_smooth(v, f))
            rows.append({"ours_s": t_o, "torch_s": t_t, "ratio": t_t / t_o})
            print(key, rows[-1], flush=True)
        _, counts = consumers.smooth_mesh(v, f, return_counts=True)
        again = torch_smooth(v, f)
        out[key] = {"alternating_pairs": rows, "V": v.shape[0], "F": f.shape[0], "counts_invalid_null_over_cap_unreferenced": counts,
                    "faster_than_torch_in_every_pair": all(x["ratio"] > 1 for x in rows), "smallest_ratio": min(x["ratio"] for x in rows),
                    "largest_difference_to_torch": float((ours - theirs).abs().max()), "largest_move": float((ours - v).abs().max()),
                    "ours_same_bytes_in_every_call": bool(torch.equal(ours, consumers.smooth_mesh(v, f))),
                    "torch_same_bytes_in_two_calls": bool(torch.equal(theirs, again))}
        print(key, {k: x for k, x in out[key].items() if k != "alternating_pairs"}, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
