"""The mesh repair on the device (consumers.repair_mesh -> dgs_mesh_repair_count / _emit, csrc/mesh_repair.hip) against the first step
of the host path it replaces: vertices.cpu().numpy(), faces.cpu().numpy() of the same mesh, which is what a user hands to pymeshlab's
four filters.  pymeshlab is not installed here, so that copy is the only part of the host path that can be timed; the filters
themselves come on top of it.
    R = 256, nb = 64, N = 262,144    the pipeline's setting: the mesh after the component filters (about 1.57 M faces) and that mesh
                                     decimated to the reference's 1e5 faces (about 99 k)
--pairs alternating pairs (ours, copy) per mesh inside one process; wall time around a device synchronisation; `ours` is the whole
call: workspace and output allocation, the analysis, the readback of the ten counts, the emit.  The census of each mesh before and
after the repair (consumers.mesh_topology) is written down with it.  Writes profiles/mesh_repair_bench.json.
    python tools/mesh_repair_bench.py [--pairs 5] [--out profiles/mesh_repair_bench.json]
    python tools/mesh_repair_bench.py --only-ours N [--mesh NAME]    N calls of ours and nothing else (the target of a rocprofv3
                                                                     --kernel-trace --stats run)
    python tools/mesh_repair_bench.py --extract-only LABEL --out FILE   extract_mesh() with its default arguments at R = 256 and R = 128,
                                                                     --pairs calls twice over (an A/A pair of medians), appended to
                                                                     FILE under LABEL: run once with this tree's library and once with
                                                                     DGS_AMD_LIBRARY = the parent's
    python tools/mesh_repair_bench.py --kernel-stats TXT --mesh NAME --calls N --out FILE   no GPU: adds to FILE each kernel's time in TXT
                                                                     per repair_mesh call
    python tools/mesh_repair_bench.py --ab-summary --out FILE        no GPU: the ratio of the medians (this / parent) of the
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_smooth_bench import LEVEL, MIN_D, MIN_F, SETTINGS, TARGET, add_ab_summary  # noqa: E402

MESHES = ("decimated", "undecimated")
KERNELS = ("rep_face_kernel", "rep_edge_insert_kernel", "rep_edge_second_kernel", "rep_edge_mark_kernel", "rep_fan_kernel", "rep_flatten_kernel",
           "rep_cscan_kernel", "rep_vscan_kernel", "rep_fscan_kernel", "rep_sums_kernel", "rep_emit_vertices_kernel", "rep_emit_faces_kernel")


def add_kernel_stats(args):
    out = json.load(open(args.out))
    s = out[args.mesh]
    rows, mine = {}, True
    for line in open(args.kernel_stats):
        if line.startswith("#"):                                              # one section a mesh, headed by the command that made it
            mine = "--mesh " + args.mesh in line
        for name in KERNELS:
            if mine and (line.startswith("dgs::" + name + "(") or line.startswith("void dgs::" + name + "<")):
                calls, total_us, avg_us = line.split()[-6:-3]                  # ... calls total_us avg_us min_us max_us pct
                row = rows.setdefault(name, {"launches": 0, "us_per_repair_mesh_call": 0.0})
                row["launches"] += int(calls)
                row["us_per_repair_mesh_call"] += float(total_us) / args.calls
    s["kernels"] = rows
    s["kernels_source"] = os.path.relpath(args.kernel_stats, ROOT) + f" (rocprofv3 --kernel-trace --stats, a run of its own, {args.calls} repair_mesh calls, the warm-up among them)"
    s["kernels_us_per_call"] = sum(r["us_per_repair_mesh_call"] for r in rows.values())
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--mesh", default=None, choices=MESHES)
    ap.add_argument("--extract-only", default=None, metavar="LABEL")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--ab-summary", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_repair_bench.json"))
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
        consumers.repair_mesh(v, f)                                           # warm-up
    if args.only_ours:
        for _ in range(args.only_ours):
            for v, f in meshes.values():
                consumers.repair_mesh(v, f)
        torch.cuda.synchronize()
        return
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out.update({"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each",
                "setting": name, "min_f": MIN_F, "min_d": MIN_D, "target_faces": TARGET,
                "ours": "consumers.repair_mesh(vertices, faces): allocation, the analysis, the readback of ten counts, the emit",
                "comparator": "vertices.cpu().numpy(), faces.cpu().numpy(): the copy in front of pymeshlab's four filters, which are not "
                              "installed here and are not timed"})
    for key, (v, f) in meshes.items():
        rows = []
        for _ in range(args.pairs):
            ours, t_o = timed(lambda: consumers.repair_mesh(v, f))
            _, t_c = timed(lambda: (v.cpu().numpy(), f.cpu().numpy()))
            rows.append({"ours_s": t_o, "copy_s": t_c, "ratio": t_c / t_o})
            print(key, rows[-1], flush=True)
        ov, of, counts = consumers.repair_mesh(v, f, return_counts=True)
        again = consumers.repair_mesh(v, f)
        out[key] = {"alternating_pairs": rows, "V": v.shape[0], "F": f.shape[0], "counts": counts,
                    "census_before": consumers.mesh_topology(v, f), "census_after": consumers.mesh_topology(ov, of),
                    "median_ours_s": statistics.median(x["ours_s"] for x in rows), "median_copy_s": statistics.median(x["copy_s"] for x in rows),
                    "faster_than_the_copy_in_every_pair": all(x["ratio"] > 1 for x in rows), "smallest_ratio": min(x["ratio"] for x in rows),
                    "workspace_bytes": consumers._repair_call(v, f, None, "bench").a.workspace_bytes,
                    "ours_same_bytes_in_every_call": bool(torch.equal(ov.view(torch.int32), again[0].view(torch.int32)) and torch.equal(of, again[1]))}
        print(key, {k: x for k, x in out[key].items() if k != "alternating_pairs"}, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
