"""What the rasterizer's depth / alpha maps cost (forward_views(aux=True), backward_views(grad_depth=, grad_alpha=)) against the
workaround they replace -- a second render of the same Gaussians with colors_precomp = (z, 1, 0) on background 0, one set per view --
and what the default (colour-only) call costs against another build of the library (the parent commit's), both loaded side by side
(with --base also: are the default colour and the deterministic form's gradients the base build's, bit for bit).
    python tools/raster_aux_bench.py [--base <other libdgs_hip.so>] [--pairs 20] [--out profiles/raster_aux_bench.json]
Every comparison alternates its two sides inside one process, a pair at a time, each side between device events; an A/A series (the
base build against itself, or the product build when no base is given) measures the spread of such pairs on the box.  The structural
condition -- an aux call is cheaper than the workaround in EVERY pair -- is checked: exit status 1 if it does not hold."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open-diffusiongs_amd"))

import numpy as np
import torch

from dgs_amd import _native, synth
from dgs_amd.raster import RasterBackend

DEV = torch.device("cuda:0")
SHAPES = [(256, 4, "trained"), (256, 4, "init"), (512, 4, "trained")]


class Scene:
    def __init__(self, res, views, regime):
        self.res, self.V = res, views
        sc = synth.gaussian_scene(res, regime=regime, seed=0)
        cams, _, _ = synth.render_cameras(res, views, phase_deg=10)
        t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=DEV)
        self.xyz, self.shs, self.sca, self.rot, self.op = (t(sc[k]) for k in ("xyz", "shs", "scales", "rotations", "opacities"))
        self.vm = t(np.stack([c["viewmatrix"] for c in cams])); self.pm = t(np.stack([c["projmatrix"] for c in cams]))
        self.cp = t(np.stack([c["campos"] for c in cams]))
        self.tan = (cams[0]["tanfovx"], cams[0]["tanfovy"])
        self.white, self.black = torch.ones(3, device=DEV), torch.zeros(3, device=DEV)
        self.P = int(self.xyz.shape[0])
        # the workaround's inputs, made once outside every timed window (generous to the workaround): one set per view, colours (z, 1, 0)
        m = self.vm.reshape(views, 16)
        z = m[:, 2:3] * self.xyz[None, :, 0] + m[:, 6:7] * self.xyz[None, :, 1] + m[:, 10:11] * self.xyz[None, :, 2] + m[:, 14:15]
        self.zcol = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], dim=2).contiguous()
        rep = lambda a: a[None].expand(views, *a.shape).contiguous()
        self.xyz_v, self.sca_v, self.rot_v, self.op_v = rep(self.xyz), rep(self.sca), rep(self.rot), rep(self.op)
        g = torch.Generator(device=DEV).manual_seed(0)
        self.dpix = torch.randn(views, 3, res, res, device=DEV, generator=g) / (3 * res * res)
        self.gD = torch.randn(views, 1, res, res, device=DEV, generator=g) / (res * res)
        self.gA = torch.randn(views, 1, res, res, device=DEV, generator=g) / (res * res)
        self.cap = self.cap_v = 0

    # one Gaussian set, all views (the product's call); cap: binning capacity of the asynchronous form (0: the synchronous form)
    def fwd(self, be, cap, **kw):
        return be.forward_views(self.white, self.xyz[None], None, self.op, self.sca[None], self.rot[None], 1.0, None, self.vm, self.pm, self.cp, None,
                                self.tan[0], self.tan[1], self.res, self.res, self.shs[None], 0, False, False, views_per_set=self.V,
                                binning_capacity=cap, **kw)

    def bwd(self, be, st, **kw):
        return be.backward_views(self.white, self.xyz[None], st[2], None, self.op, self.sca[None], self.rot[None], 1.0, None, self.vm, self.pm,
                                 self.cp, None, self.tan[0], self.tan[1], self.dpix, self.shs[None], 0, st[3], st[0], st[4], st[5], False,
                                 views_per_set=self.V, **kw)

    # the workaround's second render: a set per view, precomputed colours
    def fwd_z(self, be, cap):
        return be.forward_views(self.black, self.xyz_v, self.zcol, self.op_v, self.sca_v, self.rot_v, 1.0, None, self.vm, self.pm, self.cp, None,
                                self.tan[0], self.tan[1], self.res, self.res, None, 0, False, False, views_per_set=1, binning_capacity=cap)

    def bwd_z(self, be, st):
        g = torch.cat([self.gD, self.gA, torch.zeros_like(self.gD)], dim=1)
        return be.backward_views(self.black, self.xyz_v, st[2], self.zcol, self.op_v, self.sca_v, self.rot_v, 1.0, None, self.vm, self.pm, self.cp,
                                 None, self.tan[0], self.tan[1], g, None, 0, st[3], st[0], st[4], st[5], False, views_per_set=1)


def pairs(fa, fb, n, warm=3):
    """n alternating (a, b) pairs, each side between two device events -> (ms of a, ms of b) lists."""
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(n)]
    for e in ev:
        e[0].record(); fa(); e[1].record()
        e[2].record(); fb(); e[3].record()
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1]) for e in ev], [e[2].elapsed_time(e[3]) for e in ev]


def stats(a, b):
    r = sorted(x / y for x, y in zip(a, b))
    med = lambda v: sorted(v)[len(v) // 2]
    return dict(a_ms_median=round(med(a), 4), b_ms_median=round(med(b), 4), ratio_min=round(r[0], 4), ratio_median=round(med(r), 4),
                ratio_max=round(r[-1], 4), pairs=len(a), a_cheaper_in_every_pair=bool(r[-1] < 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=None, help="another build of libdgs_hip.so (the parent commit's) for the default-call comparison")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_aux_bench.json"))
    a = ap.parse_args()
    new = RasterBackend()
    base = RasterBackend(lib=_native.open_library(os.path.abspath(a.base))) if a.base else None
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, pairs=a.pairs,
               base_library=("another build, --base" if a.base else None),
               note="ms per call between device events; a = first side named, b = second; ratio = a / b per alternating pair", shapes=[])
    ok = True
    for res, views, regime in SHAPES:
        s = Scene(res, views, regime)
        n = int(s.fwd(new, 0)[0]); nz = int(s.fwd_z(new, 0)[0])
        cap, cap_z = int(1.2 * n), int(1.2 * nz)
        row = dict(res=res, views=views, regime=regime, P=s.P, instances=n)
        # ---- aux call against the workaround ----
        f_aux = lambda: s.fwd(new, cap, aux=True)
        f_two = lambda: (s.fwd(new, cap), s.fwd_z(new, cap_z))

        def fb_aux():
            st = s.fwd(new, cap, aux=True)
            s.bwd(new, st, grad_depth=s.gD, grad_alpha=s.gA)

        def fb_two():
            st = s.fwd(new, cap); s.bwd(new, st)
            sz = s.fwd_z(new, cap_z); s.bwd_z(new, sz)

        row["forward: aux call vs colour render + (z, 1, 0) render"] = stats(*pairs(f_aux, f_two, a.pairs))
        row["forward + backward: aux call vs the two forward + backward calls"] = stats(*pairs(fb_aux, fb_two, a.pairs))
        ok = ok and all(row[k]["a_cheaper_in_every_pair"] for k in list(row) if isinstance(row[k], dict))
        # ---- what the maps add to a call ----
        f_col = lambda: s.fwd(new, cap)

        def fb_col():
            st = s.fwd(new, cap); s.bwd(new, st)

        row["forward: aux call vs colour-only call"] = stats(*pairs(f_aux, f_col, a.pairs))
        row["forward + backward: aux call vs colour-only call"] = stats(*pairs(fb_aux, fb_col, a.pairs))
        # ---- the default call: this build against the base build, and the box's A/A spread ----
        ref = base if base is not None else new
        f_ref = lambda: s.fwd(ref, cap)

        def fb_ref():
            st = s.fwd(ref, cap); s.bwd(ref, st)

        row["A/A forward: base vs base"] = stats(*pairs(f_ref, f_ref, a.pairs))
        row["A/A forward + backward: base vs base"] = stats(*pairs(fb_ref, fb_ref, a.pairs))
        if base is not None:
            col_new, col_base = s.fwd(new, cap)[1], s.fwd(base, cap)[1]
            row["default colour bit-identical with base"] = bool(torch.equal(col_new, col_base))

            def det_grads(be, **kw):            # the deterministic backward is reproducible: the two builds must agree bit for bit
                be.deterministic = True
                g = s.bwd(be, s.fwd(be, cap, aux=bool(kw)), **kw)
                det, be.deterministic = be.last_backward_deterministic, False
                return g if det else {}

            for what, kw in (("", {}), (" with the maps", dict(grad_depth=s.gD, grad_alpha=s.gA))):
                gn, gb = det_grads(new, **kw), det_grads(base, **kw)
                row[f"deterministic gradients{what} bit-identical with base"] = bool(gn) and all(torch.equal(gn[k], gb[k]) for k in gn if gn[k] is not None)
            for what, fa, fb, aa in (("forward", f_col, f_ref, "A/A forward: base vs base"),
                                     ("forward + backward", fb_col, fb_ref, "A/A forward + backward: base vs base")):
                st_ = stats(*pairs(fa, fb, a.pairs))
                st_["inside_aa_spread"] = bool(row[aa]["ratio_min"] <= st_["ratio_median"] <= row[aa]["ratio_max"])
                row[f"default {what}: this build vs base"] = st_
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del s
        torch.cuda.empty_cache()
    out["aux_cheaper_than_workaround_in_every_pair"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}; aux cheaper than the workaround in every pair: {ok}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
