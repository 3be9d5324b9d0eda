"""Depth / alpha maps of the rasterizer (dgs_raster.h `out_depth`, `out_alpha`, `dL_ddepth`, `dL_dalpha`) against the CPU oracle, which
knows nothing of them, through one identity: a render of ONE set per view with colors_precomp = (z, 1, 0) and background 0 has
depth in colour channel 0 and alpha in channel 1 -- the pairs that blend, the 1/255 cut and the T < 1e-4 termination do not depend on the
colour -- and its backward with dL_dpix = (gD, gA, 0) gives every aux gradient: dL_dcolors[:, 0] is dL/dz, whose way into dL_dmeans3D
(the z row of the view matrix) is added here.  By linearity a call with colour and aux gradients together equals the sum of the two
oracle runs.  Bars: the forward rule of parity_util.assert_forward_parity scaled by the map's max; raster_bwd_util.close for gradients."""
import numpy as np
import torch

from oracle.raster_oracle import RasterOracle
from parity_util import exp_mode
from raster_bwd_util import NAMES, OBSERVED, close
from util_scene import oracle_forward

PER_VIEW = ("means2D", "cov3D")
PER_SET = ("opacity", "means3D", "sh", "scales", "rotations")


def _t(a, device):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)


class AuxReference:
    """Oracle runs of one scene (one Gaussian set, len(cams) views), made once and shared by the tests that need them.  Upstream
    gradients: dpix [V,3,H,W], gD, gA [V,1,H,W], seeded."""

    def __init__(self, sc, cams, H, W, bg=(1.0, 1.0, 1.0), sh_degree=0, seed=0):
        self.sc, self.cams, self.H, self.W, self.bg, self.deg = sc, cams, H, W, tuple(bg), sh_degree
        self.V, self.P = len(cams), sc["xyz"].shape[0]
        rng = np.random.default_rng(seed)
        V = self.V
        self.dpix = rng.normal(size=(V, 3, H, W)).astype(np.float32) / (3 * H * W)
        self.gD = rng.normal(size=(V, 1, H, W)).astype(np.float32) / (H * W)
        self.gA = rng.normal(size=(V, 1, H, W)).astype(np.float32) / (H * W)
        self._maps, self._z, self._grads, self._colour = {}, None, {}, {}

    def _colour_oracle(self, v):
        """The oracle after the colour forward of view v (its exponential): kept, the colour backward and z() share it."""
        if v not in self._colour:
            o = RasterOracle()
            oracle_forward(o, self.sc, self.cams[v], self.H, self.W, bg=self.bg, sh_degree=self.deg, exp_mode=1)
            self._colour[v] = o
        return self._colour[v]

    def z(self):
        """p_view.z per (view, Gaussian): the oracle's own `depths` where the Gaussian is visible (the bits the kernels hold)."""
        if self._z is None:
            zs = []
            for v, c in enumerate(self.cams):
                o = self._colour_oracle(v)
                m = c["viewmatrix"].reshape(16)
                x = self.sc["xyz"]
                plain = (m[2] * x[:, 0] + m[6] * x[:, 1] + m[10] * x[:, 2] + m[14]).astype(np.float32)
                zs.append(np.where(o.get("radii") > 0, o.get("depths"), plain).astype(np.float32))
            self._z = zs
        return self._z

    def _aux_oracle(self, v, mode):
        o = RasterOracle()
        cols = np.stack([self.z()[v], np.ones(self.P, np.float32), np.zeros(self.P, np.float32)], axis=1)
        oracle_forward(o, self.sc, self.cams[v], self.H, self.W, bg=(0.0, 0.0, 0.0), sh_degree=0, exp_mode=mode, colors_precomp=cols, shs=None)
        return o

    def maps(self, exact):
        """(depth [V,H,W], alpha [V,H,W]) of the oracle, with its exponential of the mode."""
        mode = 1 if exact else 0
        if mode not in self._maps:
            cs = [self._aux_oracle(v, mode).get("out_color") for v in range(self.V)]
            self._maps[mode] = (np.stack([c[0] for c in cs]), np.stack([c[1] for c in cs]))
        return self._maps[mode]

    def _part(self, which):
        if which in self._grads:
            return self._grads[which]
        P, V = self.P, self.V
        M = self.sc["shs"].shape[1]
        out = {"means2D": np.zeros((V, P, 3)), "cov3D": np.zeros((V, P, 6)), "opacity": np.zeros((P, 1)), "means3D": np.zeros((P, 3)),
               "sh": np.zeros((P, M, 3)), "scales": np.zeros((P, 3)), "rotations": np.zeros((P, 4))}
        for v, c in enumerate(self.cams):
            if which == "colour":
                o = self._colour_oracle(v)
                o.backward(self.dpix[v], accum64=True)
                for k in PER_VIEW:
                    out[k][v] += o.get(NAMES[k])
                for k in PER_SET:
                    out[k] += o.get(NAMES[k]).astype(np.float64)
            else:
                o = self._aux_oracle(v, 1)
                o.backward(np.concatenate([self.gD[v], self.gA[v], np.zeros((1, self.H, self.W), np.float32)]), accum64=True)
                for k in PER_VIEW:
                    out[k][v] += o.get(NAMES[k])
                for k in ("opacity", "means3D", "scales", "rotations"):
                    out[k] += o.get(NAMES[k]).astype(np.float64)
                m = c["viewmatrix"].reshape(16).astype(np.float64)
                out["means3D"] += o.get("dL_dcolors")[:, 0:1].astype(np.float64) * np.array([m[2], m[6], m[10]])[None]
        self._grads[which] = out
        return out

    def grads(self, colour, aux):
        """fp64 sums of the oracle's gradients for dL_dpix (colour) and / or (gD, gA) (aux): per view for means2D and cov3D, summed over
        the views for the rest.  Colour + aux: the sum of the two runs (linearity)."""
        parts = [self._part(w) for w, on in (("colour", colour), ("aux", aux)) if on]
        return {k: sum(p[k] for p in parts) for k in parts[0]}


def forward(backend, ref, device, exact=None, debug=True, **kw):
    """All views of the reference's scene in ONE call; kw: aux=True / aux=False / nothing (a call that never heard of aux)."""
    sc, cams = ref.sc, ref.cams
    t = lambda a: _t(a, device)
    vm = t(np.stack([c["viewmatrix"] for c in cams])); pm = t(np.stack([c["projmatrix"] for c in cams]))
    cam = t(np.stack([c["campos"] for c in cams]))
    with exp_mode(backend, exact):
        return backend.forward_views(t(ref.bg), t(sc["xyz"])[None], None, t(sc["opacities"]), t(sc["scales"])[None], t(sc["rotations"])[None],
                                     1.0, None, vm, pm, cam, None, cams[0]["tanfovx"], cams[0]["tanfovy"], ref.H, ref.W, t(sc["shs"])[None],
                                     ref.deg, False, debug, views_per_set=ref.V, **kw)


def backward(backend, ref, device, state, dpix, exact=None, **kw):
    """Backward of `state` (a forward() tuple); kw: grad_depth / grad_alpha ([V,1,H,W] arrays or None), or nothing."""
    sc, cams = ref.sc, ref.cams
    t = lambda a: _t(a, device)
    n_total, _color, radii, geom, binning, img = state[:6]
    vm = t(np.stack([c["viewmatrix"] for c in cams])); pm = t(np.stack([c["projmatrix"] for c in cams]))
    cam = t(np.stack([c["campos"] for c in cams]))
    kw = {k: t(a) for k, a in kw.items()}
    with exp_mode(backend, exact):
        return backend.backward_views(t(ref.bg), t(sc["xyz"])[None], radii, None, t(sc["opacities"]), t(sc["scales"])[None],
                                      t(sc["rotations"])[None], 1.0, None, vm, pm, cam, None, cams[0]["tanfovx"], cams[0]["tanfovy"],
                                      t(dpix), t(sc["shs"])[None], ref.deg, geom, n_total, binning, img, True, views_per_set=ref.V, **kw)


def assert_maps(ref, depth, alpha, exact, what=""):
    """parity_util.assert_forward_parity's rule for the colour, scaled by the map's max: at most max(2, 1e-5 H W) pixels of a view off
    by more than 1e-5, none by more than 5e-3; with the oracle's exponential (exact) no pixel is excused."""
    H, W = ref.H, ref.W
    want_d, want_a = ref.maps(exact)
    allowed = 0 if exact else max(2, int(1e-5 * H * W))
    for v in range(ref.V):
        for name, got, want in (("depth", depth[v, 0], want_d[v]), ("alpha", alpha[v, 0], want_a[v])):
            got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)
            assert np.isfinite(got).all(), (name, v)
            diff = np.abs(got - want) / max(float(np.abs(want).max()), 1e-12)
            off = int((diff > 1e-5).sum())
            OBSERVED.append((f"{what} forward {name} view {v} ({'exact' if exact else 'default'} exp): {off} pixels > 1e-5", float(diff.max())))
            print(f"{what} forward {name} view {v}: max {float(diff.max()):.3e} of the map's max, {off} pixels > 1e-5 (allowed {allowed})")
            assert off <= allowed and float(diff.max()) <= 5e-3, f"{name} view {v}: {off} pixels differ by more than 1e-5 (max {float(diff.max()):.3g})"


def assert_grads(g, want, what=""):
    """Every gradient of a backward_views dict against AuxReference.grads(...): raster_bwd_util.close, 2e-4 of each tensor's max."""
    V = want["means2D"].shape[0]
    P = want["means3D"].shape[0]
    for v in range(V):
        close(g["means2D"][v].cpu().numpy(), want["means2D"][v], what=f"{what} means2D view {v}")
        close(g["cov3D"][v].cpu().numpy(), want["cov3D"][v], what=f"{what} cov3D view {v}")
    close(g["opacity"].cpu().numpy().reshape(P, 1), want["opacity"], what=f"{what} opacity")
    for k in ("means3D", "sh", "scales", "rotations"):
        close(g[k][0].cpu().numpy(), want[k], what=f"{what} {k}")


def same_bits(a, b, what="", bitwise=True):
    """Two backward_views dicts that made the same arithmetic: the same bits -- on the emulator, and in the deterministic form on the
    device.  The device's atomic form adds a Gaussian's tiles in the hardware's order: two runs of ONE call differ by 3e-6 ... 1.2e-5 of
    a tensor's max (profiles/r04_raster_deterministic_ab.txt; the bar of tests/test_raster_backward_gpu.py: 3e-5), so that is what
    bitwise=False asks."""
    for k in ("means2D", "cov3D", "opacity", "means3D", "sh", "scales", "rotations"):
        if bitwise:
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs"
        else:
            assert float((a[k] - b[k]).abs().max()) <= 3e-5 * float(b[k].abs().max()) + 1e-12, f"{what}: {k} differs"


def assert_aux_parity(backend, ref, device, exact, what=""):
    """The whole check of one scene in one mode of the exponential: the maps, the gradients of the maps alone (zero upstream colour
    gradient, random gD and gA), and of all three upstream gradients together.  Returns the forward state."""
    st = forward(backend, ref, device, exact=exact, aux=True)
    assert st[6].shape == (ref.V, 1, ref.H, ref.W) and st[7].shape == (ref.V, 1, ref.H, ref.W)
    assert_maps(ref, st[6], st[7], exact, what=what)
    g = backward(backend, ref, device, st, np.zeros_like(ref.dpix), exact=exact, grad_depth=ref.gD, grad_alpha=ref.gA)
    assert_grads(g, ref.grads(False, True), what=f"{what} aux only:")
    g = backward(backend, ref, device, st, ref.dpix, exact=exact, grad_depth=ref.gD, grad_alpha=ref.gA)
    assert_grads(g, ref.grads(True, True), what=f"{what} colour + aux:")
    return st


# ---- the cases both test files run (tests/test_raster_aux_emu.py on the CPU emulator, tests/test_raster_aux_gpu.py on the device) ----
def case_absent_gradient_is_zero_gradient(be, ref, device, bitwise):
    st = forward(be, ref, device, exact=True, aux=True)
    zero = np.zeros_like(ref.gD)
    same_bits(backward(be, ref, device, st, ref.dpix, exact=True, grad_alpha=ref.gA),
              backward(be, ref, device, st, ref.dpix, exact=True, grad_depth=zero, grad_alpha=ref.gA), "gD absent", bitwise)
    same_bits(backward(be, ref, device, st, ref.dpix, exact=True, grad_depth=ref.gD),
              backward(be, ref, device, st, ref.dpix, exact=True, grad_depth=ref.gD, grad_alpha=zero), "gA absent", bitwise)
    same_bits(backward(be, ref, device, st, ref.dpix, exact=True, grad_depth=None, grad_alpha=None),
              backward(be, ref, device, st, ref.dpix, exact=True), "both None", bitwise)


def case_aux_off_is_the_call_that_never_heard_of_aux(be, ref, device, exact, bitwise):
    plain = forward(be, ref, device, exact=exact)
    off = forward(be, ref, device, exact=exact, aux=False)
    on = forward(be, ref, device, exact=exact, aux=True)
    assert len(plain) == len(off) == 6 and len(on) == 8
    assert int(plain[0]) == int(off[0]) == int(on[0])
    assert torch.equal(plain[1], off[1]) and torch.equal(plain[1], on[1])          # the colour does not know about the maps
    assert torch.equal(plain[2], off[2]) and torch.equal(plain[2], on[2])
    g_plain = backward(be, ref, device, plain, ref.dpix, exact=exact)
    same_bits(g_plain, backward(be, ref, device, off, ref.dpix, exact=exact), "aux=False", bitwise)
    same_bits(g_plain, backward(be, ref, device, on, ref.dpix, exact=exact), "state of an aux forward, colour-only backward", bitwise)


def case_deterministic_form_is_bit_reproducible(be, ref, device):
    old = be.deterministic
    be.deterministic = True
    try:
        st = forward(be, ref, device, exact=False, aux=True)
        runs = [backward(be, ref, device, st, ref.dpix, exact=False, grad_depth=ref.gD, grad_alpha=ref.gA) for _ in range(2)]
        assert be.last_backward_deterministic
    finally:
        be.deterministic = old
    same_bits(runs[0], runs[1], "two runs")


def case_autograd_three_outputs(be, device, what=""):
    """render_views_autograd(aux=True) -- raw parameters, activations and their Jacobians fused in the kernels, all views and all three
    maps in one forward and ONE backward call -- against the reference call convention: torch exp / normalize / sigmoid + the drop-in
    binding per view, once for the colour and once with colors_precomp = (z, 1, 0) on background 0 for the maps, z = the view matrix's
    z row applied by torch, gradients by torch autograd.  Bar: 1e-3 of each tensor's max, what test_raster_backward_emu.py's
    test_batched_autograd_matches_dropin_binding_with_torch_activations holds this comparison to (torch's activations against the
    kernels' own sequences on top of the 2e-4 of the kernels).  The caller has made `be` the drop-in binding's backend."""
    import dgs_amd.raster as R
    import diff_gaussian_rasterization as dgr
    from dgs_amd import cameras
    from oracle import dit_oracle as D
    H = W = 32
    B, V, P = 2, 2, 150
    g = torch.Generator().manual_seed(0)
    xyz = (torch.rand(B, P, 3, generator=g) - 0.5) * 1.2
    feats = torch.rand(B, P, 1, 3, generator=g) * 3 - 1.5
    scal = torch.randn(B, P, 3, generator=g) * 0.4 - 2.6
    rot = torch.randn(B, P, 4, generator=g)
    opa = torch.randn(B, P, 1, generator=g)
    c2w = torch.tensor(np.stack([cameras.ring_cameras(V, phase_deg=30.0 * b) for b in range(B)]))
    k = torch.tensor(cameras.default_fxfycxcy(W, H)).expand(B, V, 4).contiguous()
    view, proj, campos, tanfov = D.camera_matrices(c2w, k, H, W)
    leaves = [t.clone().to(device).requires_grad_(True) for t in (xyz, feats, scal, rot, opa)]
    img, depth, alpha = R.render_views_autograd(be, *leaves, H, W, c2w.to(device), k.to(device), aux=True)
    assert img.shape == (B, V, 3, H, W) and depth.shape == alpha.shape == (B, V, 1, H, W)
    w = (torch.randn(img.shape, generator=g) / img.numel()).to(device)
    wd = (torch.randn(depth.shape, generator=g) / depth.numel()).to(device)
    wa = (torch.randn(alpha.shape, generator=g) / alpha.numel()).to(device)
    ((img * w).sum() + (depth * wd).sum() + (alpha * wa).sum()).backward()
    ref_leaves = [t.clone().to(device).requires_grad_(True) for t in (xyz, feats, scal, rot, opa)]
    view, proj, campos = view.to(device), proj.to(device), campos.to(device)
    total = 0.0
    for b in range(B):
        for v in range(V):
            x, f, s, r, o = (t[b] for t in ref_leaves)
            act = dict(scales=torch.exp(s), rotations=torch.nn.functional.normalize(r))
            tf = (float(tanfov[b, v, 0]), float(tanfov[b, v, 1]))
            rs = dgr.GaussianRasterizationSettings(H, W, tf[0], tf[1], torch.ones(3, device=device), 1.0, view[b, v], proj[b, v], 0, campos[b, v],
                                                   False, False)
            color, _ = dgr.GaussianRasterizer(rs)(x, torch.zeros_like(x, requires_grad=True), torch.sigmoid(o), shs=f, **act)
            m = view[b, v].reshape(16)
            z = m[2] * x[:, 0] + m[6] * x[:, 1] + m[10] * x[:, 2] + m[14]
            rs0 = dgr.GaussianRasterizationSettings(H, W, tf[0], tf[1], torch.zeros(3, device=device), 1.0, view[b, v], proj[b, v], 0, campos[b, v],
                                                    False, False)
            zc = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], dim=1)
            maps, _ = dgr.GaussianRasterizer(rs0)(x, torch.zeros_like(x, requires_grad=True), torch.sigmoid(o), colors_precomp=zc, **act)
            maps_d = maps.detach()
            assert float((color.detach() - img[b, v].detach()).abs().max()) < 2e-4
            assert float((maps_d[0] - depth[b, v, 0].detach()).abs().max()) < 2e-4 * float(maps_d[0].abs().max())
            assert float((maps_d[1] - alpha[b, v, 0].detach()).abs().max()) < 2e-4
            total = total + (color * w[b, v]).sum() + (maps[0] * wd[b, v, 0]).sum() + (maps[1] * wa[b, v, 0]).sum()
    total.backward()
    for a, r_, name in zip(leaves, ref_leaves, ("xyz", "features", "scaling", "rotation", "opacity")):
        close(a.grad.cpu().numpy(), r_.grad.cpu().numpy(), rtol=1e-3, what=f"{what} autograd aux {name}")


def case_autograd_unused_maps(be, device, bitwise):
    """A loss on the colour alone through the three-output call: the maps' gradients arrive absent (a colour-only backward call), the
    parameter gradients are the colour-only call's."""
    import dgs_amd.raster as R
    from dgs_amd import cameras
    H = W = 32
    g = torch.Generator().manual_seed(1)
    raw = [(torch.rand(1, 100, 3, generator=g) - 0.5) * 1.2, torch.rand(1, 100, 1, 3, generator=g), torch.randn(1, 100, 3, generator=g) * 0.4 - 2.6,
           torch.randn(1, 100, 4, generator=g), torch.randn(1, 100, 1, generator=g)]
    c2w = torch.tensor(cameras.ring_cameras(2))[None].to(device)
    k = torch.tensor(cameras.default_fxfycxcy(W, H)).expand(1, 2, 4).contiguous().to(device)
    w = torch.randn(1, 2, 3, H, W, generator=g).to(device)
    a = [t.clone().to(device).requires_grad_(True) for t in raw]
    b = [t.clone().to(device).requires_grad_(True) for t in raw]
    (R.render_views_autograd(be, *a, H, W, c2w, k) * w).sum().backward()
    (R.render_views_autograd(be, *b, H, W, c2w, k, aux=True)[0] * w).sum().backward()
    for x, y in zip(a, b):
        if bitwise:
            assert torch.equal(x.grad, y.grad)
        else:
            assert float((x.grad - y.grad).abs().max()) <= 3e-5 * float(x.grad.abs().max()) + 1e-12


def kernel_activations(raw):
    """exp / sigmoid / normalize of raw parameters by the kernels' own fp32 sequences (raster_common.h cov3d_from_scale_rot,
    raster_forward.hip preprocess_one: det_expf, the oracle's dgs_oracle_det_expf bit for bit; un-fused fp32 otherwise), so that an
    oracle run on the result sees the numbers a raw_activations call sees -- an activation that differs in its last bit moves a pair
    across the 1/255 alpha cut-off here and there, which is a difference of the inputs, not of the rasterizer."""
    from oracle.raster_oracle import det_expf
    e = np.vectorize(det_expf, otypes=[np.float32])
    one = np.float32(1.0)
    q = raw["rotations"].astype(np.float32)
    n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    nrm = np.maximum(np.sqrt(n2), np.float32(1e-12)).astype(np.float32)
    return dict(xyz=raw["xyz"], shs=raw["shs"], scales=e(raw["scales"]), rotations=(q / nrm[:, None]).astype(np.float32),
                opacities=(one / (one + e(-raw["opacities"]))).astype(np.float32))


def case_renderer_return_aux(be, device, res, V, what=""):
    """Renderer.forward(return_aux=True) on RAW parameters -- the product's path: planned asynchronous forward, cameras, activations and
    their Jacobians in the kernels, the product's exponential -- and ONE backward for a loss on all three maps.  Oracle: the same
    cameras (the backend's own matrices) and the activated scene (kernel_activations); its gradients reach the raw parameters through
    the activations' Jacobians in fp64 here (exp: s; sigmoid: o (1 - o); normalize: (g - q (q . g)) / |raw|)."""
    import types
    from dgs_amd import cameras, synth
    from dgs_amd.denoiser import Renderer
    raw = synth.gaussian_scene(res, regime="trained", seed=0, activated=False)
    act = kernel_activations(raw)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)
    c2w = t(cameras.ring_cameras(V, phase_deg=10))[None]
    k = t(cameras.default_fxfycxcy(res)).expand(1, V, 4).contiguous()
    view, proj, campos, tanfov = (x.cpu().numpy() for x in be.cameras_from_c2w(c2w, k, res, res))
    cams = [dict(viewmatrix=view[v], projmatrix=proj[v], campos=campos[v], tanfovx=float(tanfov[v, 0]), tanfovy=float(tanfov[v, 1])) for v in range(V)]
    ref = AuxReference(act, cams, res, res)
    leaves = [t(raw[n])[None].requires_grad_(True) for n in ("xyz", "shs", "scales", "rotations", "opacities")]
    r = Renderer(types.SimpleNamespace(gaussians_sh_degree=0), backend=be)
    with torch.no_grad():
        plain = r(*leaves, res, res, c2w, k)
        img0, depth0, alpha0 = r(*leaves, res, res, c2w, k, return_aux=True)
    assert torch.equal(plain, img0)                        # forward-only path: the colour does not know about the maps
    img, depth, alpha = r(*leaves, res, res, c2w, k, return_aux=True)
    assert img.shape == (1, V, 3, res, res) and depth.shape == alpha.shape == (1, V, 1, res, res)
    assert torch.equal(img.detach(), img0) and torch.equal(depth.detach(), depth0) and torch.equal(alpha.detach(), alpha0)
    assert_maps(ref, depth[0], alpha[0], exact=False, what=what)
    ((img[0] * t(ref.dpix)).sum() + (depth[0] * t(ref.gD)).sum() + (alpha[0] * t(ref.gA)).sum()).backward()
    want = ref.grads(True, True)
    got = {n: x.grad[0].double().cpu().numpy() for n, x in zip(("xyz", "features", "scaling", "rotation", "opacity"), leaves)}
    s, o = act["scales"].astype(np.float64), act["opacities"].astype(np.float64)
    rr = raw["rotations"].astype(np.float64)
    nrm = np.maximum(np.linalg.norm(rr, axis=1, keepdims=True), 1e-12)
    q = rr / nrm
    close(got["xyz"], want["means3D"], what=f"{what} xyz")
    close(got["features"], want["sh"], what=f"{what} features")
    close(got["scaling"], want["scales"] * s, what=f"{what} scaling")
    close(got["opacity"], want["opacity"] * o * (1.0 - o), what=f"{what} opacity")
    close(got["rotation"], (want["rotations"] - q * (q * want["rotations"]).sum(1, keepdims=True)) / nrm, what=f"{what} rotation")
