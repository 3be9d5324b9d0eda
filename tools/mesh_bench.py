"""Marching cubes on the device (consumers.marching_cubes -> dgs_marching_cubes_count / _emit, csrc/mesh.hip) against the step the
reference's path pays before its marching cubes even starts: `occ.detach().cpu().numpy()` of the same grid (gs_core.py:856).  Only
that step can be measured: the `mcubes` package itself is not available to the project.
    R = 256, nb = 64, N = 262,144    the pipeline's setting
    R = 128, nb = 32, N = 65,536
--pairs alternating pairs (ours, the copy) per setting inside one call; wall time around a device synchronisation.  `ours` is the whole
call: count, the {V, F} readback, the allocation of the outputs, emit.  Also: extract_fields alone, --pairs calls twice over (an A/A
pair of medians, to compare across builds with DGS_AMD_LIBRARY), and the bytes the call must move, from shapes (csrc/mesh.hip), over
its time against the copy bandwidth (6.29 TB/s).  Writes profiles/mesh_bench.json.
    python tools/mesh_bench.py [--pairs 5] [--only-ours N] [--fields-only] [--out profiles/mesh_bench.json]
--only-ours N: N calls of ours at both settings and nothing else (the target of a rocprofv3 --kernel-trace --stats run).
--fields-only: only the extract_fields timings (for the other build of an A/B).
Needs a GPU: there is no fallback."""
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
import torch

import field_util as U
from dgs_amd import consumers

COPY_BW = 6.29e12
LEVEL = 0.005
SETTINGS = (("r128_nb32_n65536", 65536, 31, 128, 32), ("r256_nb64_n262144", 262144, 21, 256, 64))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return out, time.time() - t0


def bytes_from_shapes(r, v, f):
    """csrc/mesh.hip: occ read once by count; 1 bit a sample of flags written, read by count and by emit; two 4-byte offsets a word of
    64 samples written and read; 12 B a vertex and a triangle written; the two occ samples of a crossed edge read by emit."""
    samples, words = r ** 3, r * r * ((r + 63) // 64)
    return 4 * samples + 3 * 8 * words + 2 * 8 * words + 12 * v + 12 * f + 8 * v


def fields(models, pairs):
    out = {}
    for name, _, _, r, nb in SETTINGS:
        runs = [[timed(lambda: consumers.extract_fields(models[name], r, nb))[1] for _ in range(pairs)] for _ in range(2)]
        out[name] = {"extract_fields_s": runs, "medians_s": [statistics.median(x) for x in runs]}
        print(name, "extract_fields", out[name]["medians_s"], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--fields-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    models = {name: U.make_model(U.make_scene(n, seed), dev) for name, n, seed, _, _ in SETTINGS}
    occs = {}
    for name, _, _, r, nb in SETTINGS:                                         # warm-up: library load, allocator
        occs[name] = consumers.extract_fields(models[name], r, nb)
        if not args.fields_only:
            consumers.marching_cubes(occs[name], LEVEL)
    out = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("DGS_AMD_LIBRARY", "product"),
           "timing": "wall seconds around a device synchronisation, one call each"}
    if args.only_ours:
        for _ in range(args.only_ours):
            for name in occs:
                consumers.marching_cubes(occs[name], LEVEL)
        torch.cuda.synchronize()
        return
    if not args.fields_only:
        for name, _, _, r, _ in SETTINGS:
            occ, rows = occs[name], []
            for _ in range(args.pairs):
                (v, f), t_o = timed(lambda: consumers.marching_cubes(occ, LEVEL))
                _, t_c = timed(lambda: occ.detach().cpu().numpy())
                rows.append({"ours_s": t_o, "copy_to_host_s": t_c, "ratio": t_c / t_o})
                print(name, rows[-1], flush=True)
            best = min(x["ours_s"] for x in rows)
            moved = bytes_from_shapes(r, v.shape[0], f.shape[0])
            out[name] = {"alternating_pairs": rows, "V": v.shape[0], "F": f.shape[0], "faster_than_the_copy_in_every_pair": all(x["ratio"] > 1 for x in rows),
                         "bytes_from_shapes": moved, "grid_bytes": 4 * r ** 3, "share_of_copy_bandwidth_whole_call": moved / best / COPY_BW}
    out["extract_fields_alone"] = fields(models, args.pairs)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
