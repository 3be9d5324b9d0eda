"""The mesh decimation on the device (consumers.decimate_mesh -> dgs_mesh_decimate_count / _emit, csrc/mesh_decimate.hip) against the
step any host decimator pays before it starts: `vertices.cpu().numpy(), faces.cpu().numpy()` of the same mesh.  Only that step can be
measured: pymeshlab, whose decimate_mesh this stands in for, is not available to the project.
    R = 256, nb = 64, N = 262,144    the pipeline's setting
    R = 128, nb = 32, N = 65,536
The mesh is extract_mesh's after the component filters: marching cubes at 0.005, rescaled to [-1, 1]^3, min_f = 64, min_d = 20; the
target is the reference's 1e5 faces.
--pairs alternating pairs (ours, the copy) per setting inside one call; wall time around a device synchronisation.  `ours` is the whole
call: the bisection over n (ten or eleven counts with a readback of five integers each), the allocation of the outputs, emit.  Writes
profiles/mesh_decimate_bench.json.
    python tools/mesh_decimate_bench.py [--pairs 5] [--out profiles/mesh_decimate_bench.json]
    python tools/mesh_decimate_bench.py --only-ours N [--setting NAME]  N calls of ours and nothing else timed (the target of a
                                                                        rocprofv3 --kernel-trace --stats run)
    python tools/mesh_decimate_bench.py --extract-only LABEL --out FILE extract_mesh() with its default arguments, --pairs calls twice over
                                                                        (an A/A pair of medians), appended to FILE under LABEL: run once with
                                                                        this tree's library and once with DGS_AMD_LIBRARY = the parent's
    python tools/mesh_decimate_bench.py --kernel-stats TXT --setting NAME --calls N --out FILE   no GPU: adds to FILE each kernel's time in
                                                                        TXT per decimate_mesh call and, for the kernels whose work
                                                                        does not depend on n, its bytes from shapes against the copy bandwidth
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
LEVEL, MIN_F, MIN_D, TARGET = 0.005, 64, 20, 1e5
SETTINGS = (("r128_nb32_n65536", 65536, 31, 128, 32), ("r256_nb64_n262144", 262144, 21, 256, 64))
KERNELS = ("dec_ref_kernel", "dec_box_kernel", "dec_params_kernel", "dec_cell_kernel", "dec_occ_kernel", "dec_occ_sums_kernel", "dec_rank_kernel",
           "dec_insert_kernel", "dec_fscan_kernel", "dec_uscan_kernel", "dec_sums_kernel", "dec_accumulate_kernel", "dec_emit_vertices_kernel",
           "dec_emit_faces_kernel")


def kernel_bytes(V, F, V2, F2):
    """Bytes a launch must move at the least, from shapes (csrc/mesh_decimate.hip), for the kernels whose work does not depend on n:
    every array read or written once, 4 B a word, gathers through an index counted as 4 B each."""
    return {
        "dec_ref_kernel": 12 * F + 12 * F,                                    # faces read, ref written
        "dec_box_kernel": 4 * V + 12 * V,                                     # ref, vertices
        "dec_cell_kernel": 4 * V + 12 * V + 4 * V + 8 * V,                    # ref, vertices, vrank written, a mask word
        "dec_rank_kernel": 4 * V + 4 * V + 8 * V + 8 * V + 8 * V,             # ref, vrank read and written, two prefixes, a mask word at least, cellof
        "dec_insert_kernel": 12 * F + 12 * F + 4 * F,                         # faces, three ranks, fslot written (table traffic on top)
        "dec_fscan_kernel": 4 * F + 4 * F + 4 * F,                            # fslot, the slot, foff
        "dec_accumulate_kernel": 4 * V + 4 * V + 4 * V + 12 * V + 28 * V,     # ref, vrank, used, vertices, four atomic adds
        "dec_emit_faces_kernel": 8 * F + 4 * F + 12 * F2 + 24 * F2 + 12 * F2,  # fslot / slot, foff; faces, ranks and offsets, rows written
    }


def add_kernel_stats(args):
    out = json.load(open(args.out))
    s = out[args.setting]
    moved = kernel_bytes(s["V"], s["F"], s["V_out"], s["F_out"])
    rows = {}
    for line in open(args.kernel_stats):
        for name in KERNELS:
            if line.startswith("dgs::" + name + "("):
                calls, total_us, avg_us = line.split()[-6:-3]                  # ... calls total_us avg_us min_us max_us pct
                rows[name] = {"launches": int(calls), "avg_us": float(avg_us), "us_per_decimate_mesh_call": float(total_us) / args.calls}
                if name in moved:
                    rows[name]["bytes_from_shapes"] = moved[name]
                    rows[name]["share_of_copy_bandwidth"] = moved[name] / (float(avg_us) * 1e-6) / COPY_BW
    s["kernels"] = rows
    s["kernels_source"] = os.path.relpath(args.kernel_stats, ROOT) + f" (rocprofv3 --kernel-trace --stats, a run of its own, {args.calls} decimate_mesh calls and the warm-up)"
    s["kernel_time_us_per_decimate_mesh_call"] = sum(r["us_per_decimate_mesh_call"] for r in rows.values())
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
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate_bench.json"))
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
        mesh = models[name].extract_mesh(LEVEL, r, nb, min_f=MIN_F, min_d=MIN_D)
        meshes[name] = (mesh.vertices, mesh.faces)
        consumers.decimate_mesh(mesh.vertices, mesh.faces, TARGET)            # warm-up
    if args.only_ours:
        for _ in range(args.only_ours):
            for name in meshes:
                consumers.decimate_mesh(*meshes[name], TARGET)
        torch.cuda.synchronize()
        return
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out.update({"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each",
                "min_f": MIN_F, "min_d": MIN_D, "target_faces": TARGET,
                "ours": "consumers.decimate_mesh(vertices, faces, 1e5): the bisection over n (every count with its readback), allocation, emit",
                "comparator": "vertices.cpu().numpy(), faces.cpu().numpy() of the same mesh: the step a host decimator pays before it starts; "
                              "pymeshlab itself is not available, so its decimation is not timed"})
    for name in meshes:
        v, f = meshes[name]
        rows = []
        for _ in range(args.pairs):
            (dv, df, n), t_o = timed(lambda: consumers.decimate_mesh(v, f, TARGET, return_n=True))
            _, t_c = timed(lambda: (v.cpu().numpy(), f.cpu().numpy()))
            rows.append({"ours_s": t_o, "copy_to_host_s": t_c, "ratio": t_c / t_o})
            print(name, rows[-1], flush=True)
        counts = consumers.cluster_vertices(v, f, n, return_counts=True)[2]
        _, t_one = timed(lambda: consumers.cluster_vertices(v, f, n))
        out[name] = {"alternating_pairs": rows, "V": v.shape[0], "F": f.shape[0], "n": n, "V_out": dv.shape[0], "F_out": df.shape[0],
                     "counts_V_F_degenerate_duplicates_invalid": counts, "cluster_vertices_at_n_s": t_one,
                     "faster_than_the_copy_in_every_pair": all(x["ratio"] > 1 for x in rows), "mesh_bytes": 12 * (v.shape[0] + f.shape[0])}
        assert df.shape[0] == counts[1] <= TARGET and dv.shape[0] == counts[0]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
