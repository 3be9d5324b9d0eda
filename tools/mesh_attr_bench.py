"""Mesh attributes on the device (consumers.mesh_attributes -> dgs_mesh_attributes, csrc/mesh_attr.hip) against the same three outputs
written with torch ops on the same GPU: a dense [chunk, N] evaluation over chunks of points -- every Gaussian for every point, which is
what a user would write without the cells.
    R = 256, nb = 64, N = 262,144    the pipeline's setting, bench's shell scene (tests/field_util.py make_scene)
    R = 128, nb = 32, N = 65,536
At each, two meshes: extract_mesh's after the component filters (min_f = 64, min_d = 20) and the same decimated to 1e5 faces; reach = 2.
--pairs alternating pairs (ours, torch form) per mesh inside one call; wall time around a device synchronisation.  `ours` is the whole
mesh_attributes call (normalisation, allocation, the C call, the normals).  A torch-form call stops after --limit seconds and is then
reported as points done / seconds spent and scaled to the whole mesh (the field bench's way with its torch form).  The two forms are
compared on the points the torch form finished: they differ by the far Gaussians the window drops (and by fp32 summation order), reported
against the colour's range [0, 1] and the density level.  Pairs per second and the share of the fp32 VALU peak come from the
(point, member) pairs counted out of the two cell histograms and 45 VALU lane operations a pair (csrc/mesh_attr.hip); 157.3 TFLOP/s =
78.65e12 lane operations/s.  Writes profiles/mesh_attr_bench.json.
    python tools/mesh_attr_bench.py [--pairs 5] [--limit 20] [--out profiles/mesh_attr_bench.json]
    python tools/mesh_attr_bench.py --only-ours N     N calls of ours per mesh and nothing else timed (the target of a
                                                      rocprofv3 --kernel-trace --stats run)
    python tools/mesh_attr_bench.py --extract-only LABEL --out FILE   extract_fields and extract_mesh() with their default arguments,
                                                      --pairs calls twice over (an A/A pair of medians), appended to FILE under LABEL:
                                                      run once with this tree's library and once with DGS_AMD_LIBRARY = the parent's
Against the window's own definition the call is checked on 2,048 sampled points per mesh with the fp64 restatement of
tests/mesh_attr_util.py (the largest absolute differences are written next to the ones against the dense form).
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
import mesh_attr_util as M
from dgs_amd import consumers

VALU_LANE_OPS, OPS_PER_PAIR = 78.65e12, 45
LEVEL, MIN_F, MIN_D, TARGET, REACH = 0.005, 64, 20, 1e5, 2
SETTINGS = (("r128_nb32_n65536", 65536, 31, 128, 32), ("r256_nb64_n262144", 262144, 21, 256, 64))


def torch_form(pc, points, limit, elements=1 << 26):
    """density, colours and normals of every Gaussian at every point, fp32, in chunks of points -> (dict, points done, seconds)."""
    xyz = pc.get_xyz.float()
    mn, mx = xyz.amin(0), xyz.amax(0)
    scale = 1.8 / (mx - mn).amax().item()
    c = (xyz - (mn + mx) / 2) * scale
    g = dict(xyz=c, scaling=pc._scaling, rotation=pc._rotation, opacity=pc._opacity, mesh_scale=scale, scaling_modifier=1.0)
    co, op = M.coefficients(g, torch.float32)
    A, B, C, D, E, F = (co[:, k][None] for k in range(6))
    attr = (0.5 + consumers.C0 * pc._features_dc.float().reshape(-1, 3)).clamp(0, 1)
    V, N = points.shape[0], c.shape[0]
    step = max(1, elements // N)
    den, col, grad = (torch.zeros(V, k, device=points.device) for k in (1, 3, 3))
    done, t0 = 0, time.time()
    for v0 in range(0, V, step):
        p = points[v0:v0 + step]
        dx, dy, dz = (p[:, k, None] - c[None, :, k] for k in range(3))
        power = A * dx * dx + D * dy * dy + F * dz * dz + B * dx * dy + C * dx * dz + E * dy * dz
        t = op[None] * torch.where(power > 0, torch.zeros_like(power), torch.exp(power))
        den[v0:v0 + step, 0] = t.sum(1)
        col[v0:v0 + step] = t @ attr
        grad[v0:v0 + step] = torch.stack(((t * (2 * A * dx + B * dy + C * dz)).sum(1), (t * (B * dx + 2 * D * dy + E * dz)).sum(1),
                                          (t * (C * dx + E * dy + 2 * F * dz)).sum(1)), dim=1)
        done = min(V, v0 + step)
        if limit and (v0 // step) % 8 == 7:
            torch.cuda.synchronize()
            if time.time() - t0 > limit:
                break
    col = torch.where(den > 0, col / den, torch.zeros_like(col))
    norm = torch.sqrt((grad * grad).sum(1, keepdim=True))
    normals = torch.where(norm > 0, -grad / norm, torch.zeros_like(grad))
    torch.cuda.synchronize()
    return dict(density=den[:, 0], colors=col, normals=normals), done, time.time() - t0


def member_pairs(pc, points, nb, reach):
    """(point, member) pairs of the call, from the histograms of the two sets of cells."""
    xyz = pc.get_xyz.float()
    xyzs = (xyz - pc.mesh_center) * pc.mesh_scale
    hist = lambda x: torch.bincount(((M.cell(x[:, 0], nb) * nb + M.cell(x[:, 1], nb)) * nb + M.cell(x[:, 2], nb)), minlength=nb ** 3).double().reshape(1, 1, nb, nb, nb)
    k = 2 * reach + 1
    window = torch.nn.functional.avg_pool3d(hist(xyzs), k, stride=1, padding=reach, count_include_pad=True) * k ** 3
    return int((window * hist(points)).sum().round().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--limit", type=float, default=20.0)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--setting", default=None)
    ap.add_argument("--extract-only", default=None, metavar="LABEL")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_attr_bench.json"))
    args = ap.parse_args()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return out, time.time() - t0

    dev = torch.device("cuda:0")
    settings = [s for s in SETTINGS if args.setting in (None, s[0])]
    if args.extract_only:
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        for name, n, seed, r, nb in settings:
            pc = U.make_model(U.make_scene(n, seed), dev)
            row = {"library": os.path.basename(os.environ.get("DGS_AMD_LIBRARY", "product"))}
            for what, fn in (("extract_fields", lambda: pc.extract_fields(r, nb)), ("extract_mesh", lambda: pc.extract_mesh(LEVEL, r, nb))):
                fn()                                                                         # warm-up: library load, allocator
                runs = [[timed(fn)[1] for _ in range(args.pairs)] for _ in range(2)]
                row[what + "_s"], row[what + "_medians_s"] = runs, [statistics.median(x) for x in runs]
            out.setdefault("default_arguments", {}).setdefault(name, {}).setdefault(args.extract_only, []).append(row)
            print(name, args.extract_only, row["extract_fields_medians_s"], row["extract_mesh_medians_s"], flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    cases = []
    for name, n, seed, r, nb in settings:
        pc = U.make_model(U.make_scene(n, seed), dev)
        full = pc.extract_mesh(LEVEL, r, nb, min_f=MIN_F, min_d=MIN_D)
        small = pc.extract_mesh(LEVEL, r, nb, min_f=MIN_F, min_d=MIN_D, decimate_target=TARGET)
        for label, mesh in (("filtered", full), ("decimated", small)):
            consumers.mesh_attributes(pc, mesh.vertices, num_blocks=nb, reach=REACH)          # warm-up
            cases.append((f"{name}/{label}", pc, mesh.vertices, nb))
    if args.only_ours:
        for _ in range(args.only_ours):
            for _, pc, v, nb in cases:
                consumers.mesh_attributes(pc, v, num_blocks=nb, reach=REACH)
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each", "reach": REACH,
           "ours": "consumers.mesh_attributes(pc, vertices, num_blocks=nb, reach=2): the whole call, three outputs",
           "torch_form": f"dense [chunk, N] evaluation of every Gaussian at every point with torch ops, fp32, chunk * N = 2^26; stopped after {args.limit} s "
                         "and scaled to the whole mesh where it did not finish",
           "ops_per_pair": OPS_PER_PAIR, "fp32_valu_lane_ops_per_s": VALU_LANE_OPS}
    for name, pc, v, nb in cases:
        rows = []
        torch_form(pc, v[:4096], None)                                                       # warm-up
        for _ in range(args.pairs):
            ours, t_o = timed(lambda: consumers.mesh_attributes(pc, v, num_blocks=nb, reach=REACH))
            theirs, done, t_t = torch_form(pc, v, args.limit)
            rows.append({"ours_s": t_o, "torch_form_s": t_t, "torch_form_points_done": done, "torch_form_whole_mesh_s": t_t * v.shape[0] / done,
                         "ratio": t_t * v.shape[0] / done / t_o})
            print(name, rows[-1], flush=True)
        pairs = member_pairs(pc, v, nb, REACH)
        t_med = statistics.median(x["ours_s"] for x in rows)
        diff = {k: float((ours[k][:done] - theirs[k][:done]).abs().max()) for k in ("density", "colors", "normals")}
        on = theirs["density"][:done] > 0.1 * LEVEL
        diff["colors_where_density_above_a_tenth_of_the_level"] = float((ours["colors"][:done][on] - theirs["colors"][:done][on]).abs().max())
        diff["density_relative_to_the_level"] = diff["density"] / LEVEL
        pick = torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(1))[:2048].to(dev)
        g, attr = M.scene_inputs(dict(xyz=pc._xyz, scaling=pc._scaling, rotation=pc._rotation, opacity=pc._opacity, features=pc._features_dc))
        g = {k: (t.to(dev) if torch.is_tensor(t) else t) for k, t in g.items()}
        ref = M.restate(g, attr.to(dev), v[pick], nb, REACH, device=dev, pairs=1 << 26)
        norm = torch.sqrt((ref["grad"] ** 2).sum(1, keepdim=True))
        ref_n = torch.where(norm > 0, -ref["grad"] / norm, torch.zeros_like(norm))
        windowed = {"points": int(pick.numel()), "density": float((ours["density"][pick].cpu().double() - ref["density"]).abs().max()),
                    "colors": float((ours["colors"][pick].cpu().double() - ref["attr"]).abs().max()),
                    "normals": float((ours["normals"][pick].cpu().double() - ref_n).abs().max())}
        out[name] = {"V": v.shape[0], "max_abs_difference_from_the_fp64_restatement_of_the_window": windowed, "N": pc.get_xyz.shape[0], "nb": nb, "alternating_pairs": rows, "ours_median_s": t_med,
                     "faster_than_the_torch_form_in_every_pair": all(x["ratio"] > 1 for x in rows), "compared_on_points": done,
                     "max_abs_difference_window_vs_all_gaussians": diff, "colour_range": 1.0,
                     "point_member_pairs": pairs, "pairs_per_s_whole_call": pairs / t_med,
                     "share_of_fp32_valu_peak_whole_call": pairs * OPS_PER_PAIR / t_med / VALU_LANE_OPS,
                     "dense_pairs": v.shape[0] * pc.get_xyz.shape[0]}
        print(name, {k: out[name][k] for k in ("V", "ours_median_s", "point_member_pairs", "share_of_fp32_valu_peak_whole_call")}, diff, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
