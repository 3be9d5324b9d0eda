"""The mesh clean-up on the device (consumers.remove_small_components -> dgs_mesh_clean_count / _emit, csrc/mesh_clean.hip) against the
step any host cleaner pays before it starts: `vertices.cpu().numpy(), faces.cpu().numpy()` of the same mesh.  Only that step can be
measured: pymeshlab, whose two filters this replaces, is not available to the project.
    R = 256, nb = 64, N = 262,144    the pipeline's setting
    R = 128, nb = 32, N = 65,536
The mesh is extract_mesh's: marching cubes at 0.005, rescaled to [-1, 1]^3; min_f = 64, min_d = 20 (the reference's values).
--pairs alternating pairs (ours, the copy) per setting inside one call; wall time around a device synchronisation.  `ours` is the whole
call: count, the readback of the five counts, the allocation of the outputs, emit.  Writes profiles/mesh_clean_bench.json.
    python tools/mesh_clean_bench.py [--pairs 5] [--out profiles/mesh_clean_bench.json]
    python tools/mesh_clean_bench.py --only-ours N [--setting NAME]     N calls of ours and nothing else timed (the target of a
                                                                        rocprofv3 --kernel-trace --stats run)
    python tools/mesh_clean_bench.py --extract-only LABEL --out FILE    extract_mesh() with its default arguments, --pairs calls twice over
                                                                        (an A/A pair of medians), appended to FILE under LABEL: run once with
                                                                        this tree's library and once with DGS_AMD_LIBRARY = the parent's
    python tools/mesh_clean_bench.py --kernel-stats TXT --setting NAME --out FILE     no GPU: adds to FILE each kernel's bytes from shapes
                                                                        (csrc/mesh_clean.hip) over its time in TXT against the copy bandwidth
Needs a GPU except for --kernel-stats: there is no fallback."""
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
LEVEL, MIN_F, MIN_D = 0.005, 64, 20
SETTINGS = (("r128_nb32_n65536", 65536, 31, 128, 32), ("r256_nb64_n262144", 262144, 21, 256, 64))


def kernel_bytes(V, F, V2, F2):
    """Bytes each kernel must move at the least, from shapes (csrc/mesh_clean.hip): every array it reads or writes once, 4 B a word;
    gathers through an index (lab, keep, voff of a face's vertices) counted as 4 B each; the walks along links as one word each."""
    return {
        "clean_init_kernel": 36 * V,                                          # link, ref, cnt, box written
        "clean_link_kernel": 12 * F + 12 * F + 8 * F,                         # faces read, ref written, two link minima a face
        "clean_compress_kernel": 4 * V + 4 * V,                               # link read (at least), parent written
        "clean_hook_kernel": 12 * F + 12 * F,                                 # faces, the three parents read (at least)
        "clean_flatten_kernel": 4 * V + 4 * V,                                # parent read, lab written
        "clean_faces_kernel": 12 * F + 4 * F,                                 # faces, lab of the first index
        "clean_box_kernel": 4 * V + 4 * V + 12 * V,                           # ref, lab, vertices
        "clean_decide_kernel": 4 * V + 4 * V + 4 * V,                         # cnt, lab read, keep written
        "clean_vscan_kernel": 4 * V + 4 * V + 4 * V + 4 * V,                  # ref, lab, keep read, voff written
        "clean_fscan_kernel": 12 * F + 4 * F + 4 * F + 4 * F,                 # faces, lab, keep read, foff written
        "clean_emit_vertices_kernel": 16 * V + 12 * V2 + 12 * V2,             # ref, lab, keep, voff; kept rows read and written
        "clean_emit_faces_kernel": 12 * F + 12 * F + 12 * F2 + 12 * F2,       # faces, lab / keep / foff; voff of kept indices, kept rows written
    }


def add_kernel_stats(args):
    out = json.load(open(args.out))
    s = out[args.setting]
    moved = kernel_bytes(s["V"], s["F"], s["V_kept"], s["F_kept"])
    rows = {}
    for line in open(args.kernel_stats):
        for name in moved:
            if line.startswith("dgs::" + name + "("):
                calls, total_us, avg_us = line.split()[-6:-3]              # ... calls total_us avg_us min_us max_us pct
                rows[name] = {"calls": int(calls), "avg_us": float(avg_us), "bytes_from_shapes": moved[name],
                              "share_of_copy_bandwidth": moved[name] / (float(avg_us) * 1e-6) / COPY_BW}
    s["kernels"] = rows
    s["kernels_source"] = os.path.relpath(args.kernel_stats, ROOT) + " (rocprofv3 --kernel-trace --stats, a run of its own)"
    s["kernel_time_us_sum_of_averages"] = sum(r["avg_us"] for r in rows.values())
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--setting", default=None)
    ap.add_argument("--extract-only", default=None, metavar="LABEL")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args)

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
    settings = [s for s in SETTINGS if args.setting in (None, s[0])]
    models = {name: U.make_model(U.make_scene(n, seed), dev) for name, n, seed, _, _ in settings}
    if args.extract_only:
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        for name, _, _, r, nb in settings:
            models[name].extract_mesh(LEVEL, r, nb)                           # warm-up: library load, allocator
            runs = [[timed(lambda: models[name].extract_mesh(LEVEL, r, nb))[1] for _ in range(args.pairs)] for _ in range(2)]
            row = {"library": os.path.basename(os.environ.get("DGS_AMD_LIBRARY", "product")), "extract_mesh_s": runs, "medians_s": [statistics.median(x) for x in runs]}
            out.setdefault("extract_mesh_default_arguments", {}).setdefault(name, {}).setdefault(args.extract_only, []).append(row)
            print(name, args.extract_only, row["medians_s"], flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    meshes = {}
    for name, _, _, r, nb in settings:
        raw = models[name].extract_mesh(LEVEL, r, nb)
        meshes[name] = (raw.vertices, raw.faces)
        consumers.remove_small_components(raw.vertices, raw.faces, MIN_F, MIN_D)   # warm-up
    if args.only_ours:
        for _ in range(args.only_ours):
            for name in meshes:
                consumers.remove_small_components(*meshes[name], MIN_F, MIN_D)
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each",
           "min_f": MIN_F, "min_d": MIN_D,
           "comparator": "vertices.cpu().numpy(), faces.cpu().numpy() of the same mesh: the step a host cleaner pays before it starts; "
                         "pymeshlab itself is not available, so its filters are not timed"}
    for name in meshes:
        v, f = meshes[name]
        rows = []
        for _ in range(args.pairs):
            (cv, cf), t_o = timed(lambda: consumers.remove_small_components(v, f, MIN_F, MIN_D))
            _, t_c = timed(lambda: (v.cpu().numpy(), f.cpu().numpy()))
            rows.append({"ours_s": t_o, "copy_to_host_s": t_c, "ratio": t_c / t_o})
            print(name, rows[-1], flush=True)
        labels = consumers.remove_small_components(v, f, MIN_F, MIN_D, return_labels=True)[2]
        best = min(x["ours_s"] for x in rows)
        moved = sum(kernel_bytes(v.shape[0], f.shape[0], cv.shape[0], cf.shape[0]).values())
        out[name] = {"alternating_pairs": rows, "V": v.shape[0], "F": f.shape[0], "V_kept": cv.shape[0], "F_kept": cf.shape[0],
                     "components": int(torch.unique(labels).numel()), "faster_than_the_copy_in_every_pair": all(x["ratio"] > 1 for x in rows),
                     "mesh_bytes": 12 * (v.shape[0] + f.shape[0]), "bytes_from_shapes": moved,
                     "share_of_copy_bandwidth_whole_call": moved / best / COPY_BW}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
