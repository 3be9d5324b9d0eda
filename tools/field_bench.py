"""Density field (GaussianModel.extract_fields -> dgs_gaussian_field, csrc/field.hip) against the same computation written with torch
ops on the same GPU: the reference's loop over num_blocks^3 blocks restated (per block: the voxel coordinates, the member mask, a host
synchronisation on `mask.any()`, the adjugate quadratic form and the exponential over [voxels, members] in batches of 1024 members).
    R = 128, nb = 32, N = 65,536     --pairs alternating pairs (ours, torch form) inside one call
    R = 256, nb = 64, N = 262,144    the pipeline's setting: ours --pairs times; the torch form once, stopped at --limit seconds (it is
                                     262,144 host iterations) and then reported as blocks done / seconds spent
Wall time around a device synchronisation (extract_fields itself synchronises once, on mesh_scale's .item(), as the reference does).
Also: (voxel, member) pair evaluations per second against the fp32 VALU peak (23 VALU operations a pair, csrc/field.hip; 157.3 TFLOP/s
= 78.6e12 lane operations/s), and the bytes the call must move (occ written once, records written and read once, inputs) over its time
against the copy bandwidth (6.29 TB/s).  Writes profiles/field_bench.json.
    python tools/field_bench.py [--pairs 5] [--limit 240] [--only-ours N] [--out profiles/field_bench.json]
--only-ours N: N calls of ours at both settings and nothing else (the target of a rocprofv3 --kernel-trace --stats run).
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import field_util as U
from dgs_amd import consumers

VALU_LANE_OPS, OPS_PER_PAIR, COPY_BW = 78.65e12, 23, 6.29e12


def torch_form(pc, resolution, num_blocks, relax_ratio=1.5, limit=None):
    """-> (occ, blocks done, seconds).  Stops after `limit` seconds."""
    dev = pc._xyz.device
    block_size, split = 2 / num_blocks, resolution // num_blocks
    xyz = pc.get_xyz
    mn, mx = xyz.amin(0), xyz.amax(0)
    scale = 1.8 / (mx - mn).amax().item()
    xyzs = (xyz - (mn + mx) / 2) * scale
    q = pc._rotation / torch.sqrt((pc._rotation * pc._rotation).sum(dim=1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rot = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                       2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)
    L = rot * (pc.get_scaling * scale)[:, None, :]
    cov = L @ L.transpose(1, 2)
    covs = torch.stack((cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]), dim=1)
    opac = pc.get_opacity
    occ = torch.zeros([resolution] * 3, dtype=torch.float32, device=dev)
    chunks = torch.linspace(-1, 1, resolution).split(split)
    done, t0 = 0, time.time()
    for xi, xs in enumerate(chunks):
        for yi, ys in enumerate(chunks):
            for zi, zs in enumerate(chunks):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).to(dev)
                vmin, vmax = pts.amin(0) - block_size * relax_ratio, pts.amax(0) + block_size * relax_ratio
                mask = (xyzs < vmax).all(-1) & (xyzs > vmin).all(-1)
                done += 1
                if not mask.any():
                    continue
                c, o = covs[mask], opac[mask].view(1, -1)
                g = pts.unsqueeze(1) - xyzs[mask].unsqueeze(0)                                       # [M, L, 3]
                val = 0
                for s in range(0, c.shape[0], 1024):
                    gx, gy, gz = g[:, s:s + 1024, 0], g[:, s:s + 1024, 1], g[:, s:s + 1024, 2]
                    a, b, cc, d, e, f = (c[s:s + 1024, i] for i in range(6))
                    inv_det = 1 / (a * d * f + 2 * e * cc * b - e ** 2 * a - cc ** 2 * d - b ** 2 * f + 1e-24)
                    power = (-0.5 * (gx ** 2 * ((d * f - e ** 2) * inv_det) + gy ** 2 * ((a * f - cc ** 2) * inv_det) + gz ** 2 * ((a * d - b ** 2) * inv_det))
                             - gx * gy * ((e * cc - b * f) * inv_det) - gx * gz * ((e * b - cc * d) * inv_det) - gy * gz * ((b * cc - e * a) * inv_det))
                    power[power > 0] = -1e10
                    val = val + (o[:, s:s + 1024] * torch.exp(power)).sum(-1)
                occ[xi * split:(xi + 1) * split, yi * split:(yi + 1) * split, zi * split:(zi + 1) * split] = val.reshape(split, split, split)
            if limit is not None and time.time() - t0 > limit:
                torch.cuda.synchronize()
                return occ, done, time.time() - t0
    torch.cuda.synchronize()
    return occ, done, time.time() - t0


def ours(pc, resolution, num_blocks):
    torch.cuda.synchronize()
    t0 = time.time()
    occ = consumers.extract_fields(pc, resolution, num_blocks)
    torch.cuda.synchronize()
    return occ, time.time() - t0


def pair_count(pc, resolution, num_blocks, relax_ratio=1.5):
    """(voxel, member) pairs: a Gaussian is a member of a contiguous range of block indices on every axis."""
    xyzs = U.normalise(pc._xyz.float().cpu())[0]
    _, lo, hi = U.tables(resolution, num_blocks, relax_ratio)
    per_axis = [torch.searchsorted(lo, xyzs[:, a].contiguous(), right=False) - torch.searchsorted(hi, xyzs[:, a].contiguous(), right=True) for a in range(3)]
    return int((per_axis[0] * per_axis[1] * per_axis[2]).sum()) * (resolution // num_blocks) ** 3


def account(n, resolution, num_blocks, pairs, seconds):
    must_move = 4 * resolution ** 3 + 2 * 48 * n + 44 * n + 2 * 8 * n + 3 * 4 * num_blocks ** 3
    return {"pairs": pairs, "pairs_per_s": pairs / seconds, "share_of_fp32_valu_peak": pairs * OPS_PER_PAIR / seconds / VALU_LANE_OPS,
            "bytes_from_shapes": must_move, "share_of_copy_bandwidth": must_move / seconds / COPY_BW}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--only-ours", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    small, big = U.make_model(U.make_scene(65536, 31), dev), U.make_model(U.make_scene(262144, 21), dev)
    for pc, r, nb in ((small, 128, 32), (big, 256, 64)):                       # warm-up: library load, allocator
        ours(pc, r, nb)
    if args.only_ours:
        for _ in range(args.only_ours):
            ours(small, 128, 32)
            ours(big, 256, 64)
        return
    out = {"device": torch.cuda.get_device_name(0), "timing": "wall seconds around a device synchronisation, one call each"}
    rows = []
    for i in range(args.pairs):
        occ_o, t_o = ours(small, 128, 32)
        occ_t, done, t_t = torch_form(small, 128, 32)
        rows.append({"ours_s": t_o, "torch_form_s": t_t, "ratio": t_t / t_o, "max_abs_difference": float((occ_o - occ_t).abs().max())})
        print(rows[-1], flush=True)
    p = pair_count(small, 128, 32)
    out["r128_nb32_n65536"] = {"alternating_pairs": rows, "field_max": float(occ_o.max()), **account(65536, 128, 32, p, min(r["ours_s"] for r in rows))}
    times = [ours(big, 256, 64)[1] for _ in range(args.pairs)]
    print("pipeline setting, ours:", times, flush=True)
    occ_o = ours(big, 256, 64)[0]
    occ_t, done, t_t = torch_form(big, 256, 64, limit=args.limit)
    total = 64 ** 3
    covered = done // (64 * 64) * 4                                             # x slabs completed: whole (yi, zi) planes of blocks
    out["r256_nb64_n262144"] = {
        "ours_s": times, "torch_form": {"seconds": t_t, "blocks_done": done, "blocks_total": total, "finished": done == total,
                                        "seconds_for_all_blocks_at_this_rate": t_t * total / done},
        "max_abs_difference_on_finished_slabs": float((occ_o[:covered] - occ_t[:covered]).abs().max()) if covered else None,
        "field_max": float(occ_o.max()), **account(262144, 256, 64, pair_count(big, 256, 64), min(times))}
    print(out["r256_nb64_n262144"], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
