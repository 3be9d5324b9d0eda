"""Yardstick of the mesh-attribute tests: an fp64 torch restatement of include/dgs_mesh_attr.h, written from the header (the window
membership by the fp32 cell function, Sigma^-1 = R diag(1 / s^2) R^T), its fp32 evaluation with the same expressions, the raw ctypes
call with guard bands, and the bars.

Bars, per point and per component (n_p the point's member count, e32_* the fp32 restatement's largest absolute deviation from the fp64
one over the case; the factor 4 is the one of tests/field_util.py and tests/ssim_util.py):
    density   |got - ref64| <= max(4 e32_density, (n_p + 1) 2^-24 ref64)
    attr      |got - ref64| <= max(4 e32_attr,    2 (n_p + 1) 2^-24 max|attr|)     only where ref64 density >= 2^-100; below that the
              ratio lives on flushed terms and must merely be finite
    gradient  |got - ref64| <= max(4 e32_grad,    (n_p + 1) 2^-24 sum_i |t_i grad power_i|), the sum from the restatement
Reads nothing outside the repository."""
import ctypes

import numpy as np
import torch

TINY = 2.0 ** -100
GUARD = 32                     # floats on either side of every output
SENTINEL = -777.25


def cell(x, nb):
    """The header's cell of fp32 coordinates: t = floor((x + 1) * (0.5f * nb)); 0 if not t >= 0, nb - 1 if t > nb - 1, else (int)t."""
    x = x.float()
    t = torch.floor((x + 1.0) * (0.5 * nb))
    c = torch.where(t >= 0, t, torch.zeros_like(t))                          # a NaN fails the comparison
    c = torch.where(c > nb - 1, torch.full_like(c, nb - 1), c)
    return c.long()


def coefficients(g, dtype):
    """(A, B, C, D, E, F) [N, 6] of -1/2 R diag(1 / s^2) R^T with the off-diagonal ones doubled, and sigmoid(opacity) [N]."""
    rot = g["rotation"].to(dtype)
    q = rot / torch.sqrt((rot * rot).sum(dim=1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)
    mul = float(np.float32(g["scaling_modifier"])) * float(np.float32(g["mesh_scale"]))
    s = torch.exp(g["scaling"].to(dtype)) * mul
    w = -0.5 / (s * s)
    M = (R * w[:, None, :]) @ R.transpose(1, 2)
    co = torch.stack((M[:, 0, 0], 2 * M[:, 0, 1], 2 * M[:, 0, 2], M[:, 1, 1], 2 * M[:, 1, 2], M[:, 2, 2]), dim=1)
    return co, torch.sigmoid(g["opacity"].to(dtype).reshape(-1))


def restate(g, attr, points, nb, reach, dtype=torch.float64, device="cpu", pairs=2_000_000):
    """-> dict(density [V], attr [V, 3], grad [V, 3], n [V] member counts, gabs [V, 3] = sum_i |t_i grad power_i|), on the CPU.
    g: dict(xyz normalised fp32 [N, 3], scaling, rotation, opacity, mesh_scale, scaling_modifier)."""
    g = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in g.items()}
    attr, points = attr.float().to(device), points.float().to(device)
    co, op = coefficients(g, dtype)
    A, B, C, D, E, F = (co[:, k][None] for k in range(6))
    gc, c = cell(g["xyz"], nb), g["xyz"].to(dtype)
    V, N = points.shape[0], c.shape[0]
    out = dict(density=torch.zeros(V, dtype=dtype), attr=torch.zeros(V, 3, dtype=dtype), grad=torch.zeros(V, 3, dtype=dtype),
               n=torch.zeros(V, dtype=torch.int64), gabs=torch.zeros(V, 3, dtype=dtype))
    step = max(1, pairs // max(N, 1))
    for v0 in range(0, V, step):
        p = points[v0:v0 + step]
        pc = cell(p, nb)
        member = ((gc[None] - pc[:, None]).abs() <= reach).all(-1)                                  # [chunk, N]
        d = p.to(dtype)[:, None, :] - c[None]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        power = A * dx * dx + D * dy * dy + F * dz * dz + B * dx * dy + C * dx * dz + E * dy * dz
        w = torch.where(power > 0, torch.zeros_like(power), torch.exp(torch.clamp(power, min=-126.0)))
        t = torch.where(member, op[None] * w, torch.zeros_like(w))
        gp = torch.stack((2 * A * dx + B * dy + C * dz, B * dx + 2 * D * dy + E * dz, C * dx + E * dy + 2 * F * dz), dim=-1)
        gp = torch.where(member[..., None], gp, torch.zeros_like(gp))                               # a NaN point: no 0 * NaN from non-members
        den = t.sum(1)
        num = (t[..., None] * attr.to(dtype)[None]).sum(1)
        sl = slice(v0, v0 + step)
        out["density"][sl] = den.cpu()
        out["attr"][sl] = torch.where(den[:, None] > 0, num / den[:, None], torch.zeros_like(num)).cpu()
        out["grad"][sl] = (t[..., None] * gp).sum(1).cpu()
        out["gabs"][sl] = (t[..., None] * gp).abs().sum(1).cpu()
        out["n"][sl] = member.sum(1).cpu()
    return out


def raw(L, device, g, attr, points, nb, reach, want=("density", "attr", "grad"), tweak=None):
    """One dgs_mesh_attributes call with guard bands around every output -> (rc, dict of numpy outputs, dict of whole buffers).  The
    guards are asserted intact when rc == 0.  tweak(args) may spoil the arguments (the invalid-argument cases)."""
    from dgs_amd import _native
    t = lambda x: x.detach().float().contiguous().to(device)
    xyz, scaling, rotation, opacity, attr, points = (t(x) for x in (g["xyz"], g["scaling"], g["rotation"], g["opacity"].reshape(-1), attr, points))
    a = _native.DgsMeshAttrArgs()
    a.V, a.N, a.nb, a.reach = points.shape[0], xyz.shape[0], nb, reach
    a.mesh_scale, a.scaling_modifier = float(g["mesh_scale"]), float(g["scaling_modifier"])
    a.workspace_bytes = max(L.dgs_mesh_attributes_workspace_bytes(a.N, max(1, min(nb, 256)), a.V), 16)
    ws = torch.zeros(a.workspace_bytes, dtype=torch.uint8, device=device)
    widths = dict(density=1, attr=3, grad=3)
    bufs = {k: torch.full((2 * GUARD + widths[k] * a.V,), SENTINEL, dtype=torch.float32, device=device) for k in want}
    ptr = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    a.xyz, a.scaling, a.rotation, a.opacity, a.attr, a.workspace = (ptr(x) for x in (xyz, scaling, rotation, opacity, attr, ws))
    a.points = ptr(points) if a.V else None
    a.density = ptr(bufs["density"], 4 * GUARD) if "density" in want else None
    a.attr_out = ptr(bufs["attr"], 4 * GUARD) if "attr" in want else None
    a.gradient = ptr(bufs["grad"], 4 * GUARD) if "grad" in want else None
    if tweak:
        tweak(a)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream) if str(device) != "cpu" else None
    rc = L.dgs_mesh_attributes(ctypes.byref(a), stream)
    if str(device) != "cpu":
        torch.cuda.synchronize()
    whole = {k: b.cpu().numpy() for k, b in bufs.items()}
    out = {}
    for k, b in whole.items():
        if rc == 0:
            assert (b[:GUARD] == SENTINEL).all() and (b[len(b) - GUARD:] == SENTINEL).all(), f"guard band of {k} written"
        body = b[GUARD:len(b) - GUARD]
        out[k] = body.reshape(-1, 3) if widths[k] == 3 else body
    return rc, out, whole


def e32_of(g, attr, points, nb, reach, ref64, device="cpu"):
    r32 = restate(g, attr, points, nb, reach, dtype=torch.float32, device=device)
    return {k: float((r32[k].double() - ref64[k]).abs().max()) if ref64[k].numel() else 0.0 for k in ("density", "attr", "grad")}


def check_case(name, got, ref64, e32, attr, level_set, report=None):
    """got: the numpy outputs of raw(); prints the measured err / bar per output, then asserts the bars of this module's docstring and
    the share of exempted points (0 on a level set, at most 1 % elsewhere), which is a property of the restatement alone."""
    n1 = (ref64["n"].double() + 1)
    u = 2.0 ** -24
    den = torch.from_numpy(got["density"].copy()).double()
    at = torch.from_numpy(got["attr"].copy()).double()
    gr = torch.from_numpy(got["grad"].copy()).double()
    bar_d = torch.maximum(torch.full_like(n1, 4 * e32["density"]), n1 * u * ref64["density"])
    amax = float(attr.abs().max()) if attr.numel() else 0.0
    bar_a = torch.maximum(torch.full_like(n1, 4 * e32["attr"]), 2 * n1 * u * amax)[:, None]
    bar_g = torch.maximum(torch.full_like(ref64["gabs"], 4 * e32["grad"]), n1[:, None] * u * ref64["gabs"])
    live = ref64["density"] >= TINY
    exempt = float((~live).double().mean()) if live.numel() else 0.0
    err_d, err_a, err_g = (den - ref64["density"]).abs(), (at - ref64["attr"]).abs(), (gr - ref64["grad"]).abs()
    ratio = lambda e, b: float((e / b.clamp_min(1e-300)).max()) if e.numel() else 0.0
    rd, ra, rg = ratio(err_d, bar_d), ratio(err_a[live], bar_a.expand_as(err_a)[live]), ratio(err_g, bar_g)
    line = (f"{name}: V {den.numel()} members/point max {int(ref64['n'].max()) if den.numel() else 0} err/bar density {rd:.3f} attr {ra:.3f} "
            f"gradient {rg:.3f}; e32 {e32['density']:.2e} {e32['attr']:.2e} {e32['grad']:.2e}; exempt {exempt:.4f}")
    print(line)
    if report is not None:
        report.append(line)
    assert exempt == 0.0 if level_set else exempt <= 0.01, line
    assert bool(torch.isfinite(den).all() and torch.isfinite(at).all() and torch.isfinite(gr).all()), line
    assert bool((err_d <= bar_d).all()), line
    assert bool((err_a[live] <= bar_a.expand_as(err_a)[live]).all()), line
    assert bool((err_g <= bar_g).all()), line
    empty = ref64["n"] == 0
    assert bool((den[empty] == 0).all() and (at[empty] == 0).all() and (gr[empty] == 0).all()), line
    assert bool((at[den == 0] == 0).all()), line
    return rd, ra, rg


def random_scene(n, seed, spread=0.8, smin=0.05, smax=0.2):
    """n Gaussians uniform in +-spread, scales log-uniform in [smin, smax], random rotations, opacity logits in +-2, attributes in [0, 1):
    already normalised (mesh_scale 1).  Only torch.rand: the same bits on every host."""
    q = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=q, dtype=torch.float64)
    g = dict(xyz=((2 * r(n, 3) - 1) * spread).float(), scaling=(np.log(smin) + (np.log(smax) - np.log(smin)) * r(n, 3)).float(),
             rotation=(2 * r(n, 4) - 1 + 0.05).float(), opacity=(4 * r(n) - 2).float(), mesh_scale=1.0, scaling_modifier=1.0)
    return g, r(n, 3).float()


def random_points(v, seed, spread=0.9):
    q = torch.Generator().manual_seed(seed)
    return ((2 * torch.rand(v, 3, generator=q, dtype=torch.float64) - 1) * spread).float()


def scene_inputs(scene, scaling_modifier=None):
    """A scene of tests/field_util.py -> (g, attr) as mesh_attributes forms them: the reference's recentring, the degree-0 colour."""
    import field_util as FU
    xyzs, _, scale = FU.normalise(scene["xyz"].float())
    g = dict(xyz=xyzs.contiguous(), scaling=scene["scaling"], rotation=scene["rotation"], opacity=scene["opacity"], mesh_scale=scale,
             scaling_modifier=1.0 if scaling_modifier is None else scaling_modifier)
    attr = (0.5 + 0.28209479177387814 * scene["features"].float().reshape(-1, 3)).clamp(0, 1)
    return g, attr
