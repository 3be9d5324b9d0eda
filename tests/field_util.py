"""Yardstick of the density-field tests: the scene generator and an fp64 restatement of what the reference's
GaussianModel.extract_fields computes (include/dgs_field.h states it; gs_core.py:27-46, 112-147, 786-852).

Membership of a Gaussian in a block and the coordinates come from the fp32 quantities the reference forms (the normalised centres, the
linspace table, the block bounds: a hard cut by centre is part of the result); everything after that is fp64, in the reference's
adjugate form with its + 1e-24 in the determinant.  tests/golden/field_ref.npz (tools/make_field_golden.py) holds the reference's own
fp32 result of the same scenes; its distance from this restatement is `e32`.

Bound for the product, per voxel:  |got - ref64| <= max(4 * e32, (n_b + 1) * 2^-24 * ref64)
  4 * e32: the factor tests/ssim_util.py gives an fp32 evaluation in another order than the reference's;
  (n_b + 1) * 2^-24 * ref64: the worst case of adding the block's n_b non-negative fp32 terms one after the other where torch adds
  pairwise.
And the number of voxels on the other side of the mesh level 0.005 (the reference's density_thresh) is at most max(2, 1e-5 * voxels),
the form of tests/parity_util.py.  Reads nothing outside the repository."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_ref.npz")
LEVEL = 0.005
# name -> (N, resolution, num_blocks, seed, number of sampled blocks or None for the whole field)
FIXTURE_CASES = {"r32_nb8": (2000, 32, 8, 1, None), "r40_nb4": (2000, 40, 4, 2, None), "r64_nb16": (20000, 64, 16, 3, 512)}
PIPELINE_FILTERS = dict(opacity_thres=0.02, crop_bbx=[-0.91, 0.91, -0.91, 0.91, -0.91, 0.91])          # pipline_obj.py:310-316


def _gauss(shape, g):
    """Approximately N(0, 1): twelve uniforms minus six, in fp64 -- only additions, so the same bits on every host."""
    return torch.rand(*shape, 12, generator=g, dtype=torch.float64).sum(-1) - 6.0


def make_scene(n, seed):
    """Centres on a shell of radius 0.6 +- 0.03, one eighth uniform in +-1.1 (the pipeline's crop removes some of those); scales
    between 0.01 and 0.05 per axis (log-uniform, stored as logs); random quaternions; opacity logits ~N(0, 2^2).  Drawn with
    torch.rand and exactly rounded operations only (+, *, /, sqrt in fp64, one rounding to fp32), so that every host regenerates
    the bits the fixture was minted from (the fixture keeps their SHA-256).  -> dict of float32 tensors."""
    g = torch.Generator().manual_seed(seed)
    d = _gauss((n, 3), g)
    d = d / torch.sqrt((d * d).sum(dim=1, keepdim=True))
    xyz = d * (0.6 + 0.03 * (2 * torch.rand(n, 1, generator=g, dtype=torch.float64) - 1))
    k = n // 8
    xyz[:k] = (2 * torch.rand(k, 3, generator=g, dtype=torch.float64) - 1) * 1.1
    lo, hi = -4.605170185988091, -2.995732273553991                      # log 0.01, log 0.05
    scaling = lo + (hi - lo) * torch.rand(n, 3, generator=g, dtype=torch.float64)
    rotation = _gauss((n, 4), g)
    opacity = 2.0 * _gauss((n, 1), g)
    features = torch.rand(n, 1, 3, generator=g, dtype=torch.float64)
    f = lambda t: t.float().contiguous()
    return dict(xyz=f(xyz), features=f(features), scaling=f(scaling), rotation=f(rotation), opacity=f(opacity))


def scene_digest(scene):
    import hashlib
    h = hashlib.sha256()
    for k in ("xyz", "scaling", "rotation", "opacity"):
        h.update(scene[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def make_model(scene, device="cpu", scaling_modifier=None):
    from dgs_amd.denoiser import GaussianModel
    t = lambda k: scene[k].clone().to(device)
    return GaussianModel(0, scaling_modifier).set_data(t("xyz"), t("features"), t("scaling"), t("rotation"), t("opacity"))


def sample_blocks(nb, count, seed):
    """`count` distinct blocks (xi, yi, zi) of an nb^3 grid, seeded."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randperm(nb ** 3, generator=g)[:count].sort().values
    return [(int(f) // (nb * nb), (int(f) // nb) % nb, int(f) % nb) for f in flat]


def normalise(xyz):
    """The reference's recentring (gs_core.py:797-801) in fp32 -> (xyzs, mesh_center, mesh_scale)."""
    mn, mx = xyz.amin(0), xyz.amax(0)
    center = (mn + mx) / 2
    scale = 1.8 / (mx - mn).amax().item()
    return (xyz - center) * scale, center, scale


def tables(resolution, num_blocks, relax_ratio=1.5):
    """linspace / block bounds in fp32 with the reference's expressions (gs_core.py:809-824)."""
    block_size = 2 / num_blocks
    lin = torch.linspace(-1, 1, resolution)
    chunks = lin.split(resolution // num_blocks)
    lo = torch.stack([c.min() for c in chunks]) - block_size * relax_ratio
    hi = torch.stack([c.max() for c in chunks]) + block_size * relax_ratio
    return lin, lo, hi


def member_mask(xyzs, lo, hi, block):
    xi, yi, zi = block
    vmin, vmax = torch.stack((lo[xi], lo[yi], lo[zi])), torch.stack((hi[xi], hi[yi], hi[zi]))
    return (xyzs < vmax).all(-1) & (xyzs > vmin).all(-1)


def _cov6(stds, rotation):
    """(R S)(R S)^T as [a, b, c, d, e, f] in the dtype of `stds`."""
    q = rotation / torch.sqrt((rotation * rotation).sum(dim=1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)
    L = R * stds[:, None, :]
    cov = L @ L.transpose(1, 2)
    return cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]


def field_ref64(scene, resolution, num_blocks, relax_ratio=1.5, blocks=None, scaling_modifier=None, dtype=torch.float64):
    """-> (values, counts): for every block of `blocks` (default: all, in x-major order) the fp64 field of its split^3 voxels
    [n_blocks, split, split, split] and its member count [n_blocks].  dtype=torch.float32 evaluates the same expressions in fp32:
    what the reference itself computes, restated -- the source of `e32` where no fixture of the reference's output exists."""
    xyz = scene["xyz"].float().cpu()
    xyzs, _, mesh_scale = normalise(xyz)
    lin, lo, hi = tables(resolution, num_blocks, relax_ratio)
    split = resolution // num_blocks
    if blocks is None:
        blocks = [(x, y, z) for x in range(num_blocks) for y in range(num_blocks) for z in range(num_blocks)]
    mod = 1.0 if scaling_modifier is None else float(scaling_modifier)
    stds = torch.exp(scene["scaling"].to(dtype).cpu()) * mod * float(np.float32(mesh_scale))
    a, b, c, d, e, f = _cov6(stds, scene["rotation"].to(dtype).cpu())
    inv_det = 1 / (a * d * f + 2 * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + 1e-24)
    ia, ib, ic = (d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det
    id_, ie, if_ = (a * f - c ** 2) * inv_det, (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det
    op = torch.sigmoid(scene["opacity"].to(dtype).cpu()).reshape(-1)
    values = torch.zeros(len(blocks), split, split, split, dtype=dtype)
    counts = torch.zeros(len(blocks), dtype=torch.int64)
    for n, (xi, yi, zi) in enumerate(blocks):
        m = member_mask(xyzs, lo, hi, (xi, yi, zi))
        counts[n] = int(m.sum())
        if counts[n] == 0:
            continue
        xs, ys, zs = (lin[i * split:(i + 1) * split] for i in (xi, yi, zi))
        xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
        pts = torch.stack((xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)), dim=-1).to(dtype)            # [M, 3]
        g = pts[:, None, :] - xyzs[m].to(dtype)[None]                                                      # [M, L, 3]
        x, y, z = g[..., 0], g[..., 1], g[..., 2]
        power = (-0.5 * (x ** 2 * ia[m] + y ** 2 * id_[m] + z ** 2 * if_[m]) - x * y * ib[m] - x * z * ic[m] - y * z * ie[m])
        w = torch.where(power > 0, torch.zeros_like(power), torch.exp(power))
        values[n] = (op[m][None] * w).sum(-1).reshape(split, split, split)
    return values, counts


def e32_of(scene, resolution, num_blocks, ref64, **kw):
    """The fp32 restatement's largest deviation from the fp64 one (absolute)."""
    ref32, _ = field_ref64(scene, resolution, num_blocks, dtype=torch.float32, **kw)
    return float((ref32.double() - ref64).abs().max())


def gather_blocks(occ, num_blocks, blocks):
    """occ [R, R, R] -> [n_blocks, split, split, split] of the listed blocks."""
    s = occ.shape[0] // num_blocks
    return torch.stack([occ[x * s:(x + 1) * s, y * s:(y + 1) * s, z * s:(z + 1) * s] for x, y, z in blocks])


def all_blocks(num_blocks):
    return [(x, y, z) for x in range(num_blocks) for y in range(num_blocks) for z in range(num_blocks)]


def check_field(name, got, ref64, counts, e32, report=None):
    """got / ref64 [n_blocks, s, s, s], counts [n_blocks], e32 the reference's own fp32 deviation (absolute).  Prints, then asserts the
    bound of this module's docstring.  -> (max abs deviation, voxels on the other side of LEVEL)."""
    got = got.detach().cpu().double()
    err = (got - ref64).abs()
    bound = torch.maximum(torch.full_like(ref64, 4 * e32), (counts.double() + 1)[:, None, None, None] * 2.0 ** -24 * ref64)
    top = float(ref64.max())
    flips = int(((got > LEVEL) != (ref64 > LEVEL)).sum())
    cap = max(2, int(1e-5 * ref64.numel()))
    worst = float((err / bound).max())
    line = (f"{name}: max |got - ref64| {float(err.max()):.3e} = {float(err.max()) / top:.3e} of the field's max {top:.4g} "
            f"(e32 {e32 / top:.3e} of max; worst err / bound {worst:.3f}); level-{LEVEL} flips {flips} (cap {cap}); "
            f"blocks {len(counts)}, non-empty {int((counts > 0).sum())}, most members {int(counts.max())}")
    print(line)
    if report is not None:
        report.append(line)
    assert bool(torch.isfinite(got).all()), line
    assert bool((err <= bound).all()), line
    assert flips <= cap, line
    # blocks without members are exactly zero; elsewhere a zero stands only where every term is below fp32's normal range (the
    # hardware's 2^x flushes such results): ref64 <= (n_b + 1) * 2^-126
    empty = counts == 0
    assert bool((got[empty] == 0).all()), line
    assert bool((ref64[got == 0] <= ((counts.double() + 1)[:, None, None, None] * 2.0 ** -126).expand_as(ref64)[got == 0]).all()), line
    return float(err.max()), flips


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def golden_scene(name):
    """-> (scene, filtered scene): the raw inputs the fixture was minted from (stored for the small cases, regenerated and checked
    against the stored digest for the large one) and what the reference's extract_fields saw after its apply_all_filters."""
    g = golden()
    n, r, nb, seed, sampled = FIXTURE_CASES[name]
    if f"{name}/xyz" in g:
        scene = {k: torch.from_numpy(g[f"{name}/{k}"]) for k in ("xyz", "scaling", "rotation", "opacity")}
        scene["features"] = make_scene(n, seed)["features"]
    else:
        scene = make_scene(n, seed)
    assert scene_digest(scene) == str(g[f"{name}/digest"]), f"{name}: make_scene does not regenerate the fixture's inputs"
    keep = torch.from_numpy(g[f"{name}/mask_all"])
    return scene, {k: v[keep] for k, v in scene.items()}


def golden_blocks(name):
    n, r, nb, seed, sampled = FIXTURE_CASES[name]
    return all_blocks(nb) if sampled is None else [tuple(int(v) for v in b) for b in golden()[f"{name}/blocks"]]
