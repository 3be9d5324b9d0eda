"""The training objective from a clean batch: csrc/sampler.hip's dgs_train_inputs (q_sample of the noisy views, the copy of the
conditioning view and the xyz target in one launch) against the torch fp32 expressions bit for bit, and
DataParallelTrainer.configure_objective / train_step against `step()`, against an unsplit evaluation and -- on the emulator -- against
the reference's own PointDiffusionSystem.forward.

check_* take (lib, device): tests/test_train_objective_emu.py runs them on the CPU emulator build, tests/test_train_objective_gpu.py on
the GPU.  Every C-level launch writes between the guard bands of tests/step_kernels_util.py."""
import ctypes

import numpy as np
import torch

from dgs_amd import _native, cameras, denoiser as dn
from step_kernels_util import FILL, Guarded

# (B, V, H, W): copy only; one noisy view of one float4 per plane; 15 float4 (a partial workgroup); 64 float4; and a plane of
# 256 * 256 + 257 float4 -- the launch caps its grid at 256 workgroups of 256 lanes per plane (DGS_TRAIN_INPUTS_GRID_X), so the
# grid-stride loop takes a full first trip and a second one of one workgroup and one lane
SHAPES = [(1, 1, 2, 2), (2, 2, 2, 2), (3, 4, 6, 10), (2, 3, 8, 8), (2, 2, 84, 3133)]
GRID_X = 256
assert 84 * 3133 == 4 * (GRID_X * 256 + 257)
T = 1000


def _ptr(x):
    return None if x is None else ctypes.c_void_p(x.data_ptr())


def _stream(dev):
    dev = torch.device(dev)
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None


_data = {}


def kernel_data(shape):
    """CPU fp32 inputs of one shape, built once and left unchanged."""
    if shape not in _data:
        B, V, H, W = shape
        g = torch.Generator().manual_seed(1000 + 7 * len(_data))
        r = lambda *s: torch.rand(*s, generator=g)
        _data[shape] = dict(image=r(B, V, 3, H, W), noise=torch.randn(B, V, 3, H, W, generator=g), depth=1.5 + r(B, V, 1, H, W),
                            ray_o=torch.randn(B, V, 3, H, W, generator=g), ray_d=torch.randn(B, V, 3, H, W, generator=g))
    return _data[shape]


def t_mixes(B):
    """Timesteps that cover 0 and T - 1 and, where there is more than one sample, differ across the samples."""
    return {1: [[0], [T - 1]], 2: [[0, T - 1], [T - 1, 417]], 3: [[0, T - 1, 417]]}[B]


def expected(d, data, ts):
    """The reference's expressions (gaussian_diffusion.py:280-284, diffusion_gs_system.py:87-88) as separate torch fp32 ops on the CPU
    (no contraction), with the fp32 tables read back from the SpacedDiffusion object."""
    a, s = d._sqrt_acp.cpu(), d._sqrt_1m_acp.cpu()
    t = torch.tensor(ts, dtype=torch.int64)
    img = data["image"].clone()
    ca, cs = a[t].reshape(-1, 1, 1, 1, 1), s[t].reshape(-1, 1, 1, 1, 1)
    img[:, 1:] = ca * data["image"][:, 1:] + cs * data["noise"][:, 1:]
    return img, data["ray_o"] + data["ray_d"] * data["depth"]


def train_inputs_call(lib, device, d, shape, image, noise, stride, offset, t, out, depth=None, ray_o=None, ray_d=None, xyz=None, bad=None,
                      clean_views=1, tables=True, T_=None):
    B, V, H, W = shape
    a = _native.DgsTrainInputsArgs()
    a.B, a.V, a.H, a.W, a.clean_views = B, V, H, W, clean_views
    a.image, a.noise, a.noise_stride, a.noise_offset, a.t = _ptr(image), _ptr(noise), stride, offset, _ptr(t)
    if tables:
        a.sqrt_acp, a.sqrt_1m_acp = _ptr(d._sqrt_acp), _ptr(d._sqrt_1m_acp)
    a.T = d.num_timesteps if T_ is None else T_
    a.out_image, a.depth, a.ray_o, a.ray_d, a.out_gt_xyz, a.bad_t = _ptr(out), _ptr(depth), _ptr(ray_o), _ptr(ray_d), _ptr(xyz), _ptr(bad)
    return lib.dgs_train_inputs(ctypes.byref(a), _stream(device))


def _bad_flag(device):
    return Guarded(1, device, dtype=torch.int32, init=torch.zeros(1, dtype=torch.int32))


def check_train_inputs_shape(lib, device, shape):
    from dgs_amd import sampler
    lib = lib or _native.lib()
    d = sampler.create_diffusion("1000", device=device, lib=lib)
    assert d.num_timesteps == T
    B, V, H, W = shape
    data = kernel_data(shape)
    n, view = B * V * 3 * H * W, 3 * H * W
    dev = {k: v.to(device) for k, v in data.items()}
    part = data["noise"][:, 1:].contiguous().to(device)                  # the [B, V-1] draw: the same bytes, offset 0
    mixes = t_mixes(B) if H * W < 1000 else t_mixes(B)[:1]
    for ts in mixes:
        want_img, want_xyz = expected(d, data, ts)
        t = torch.tensor(ts, dtype=torch.int64, device=device)
        # A: the full draw with an offset of one view, with depth, into fresh buffers
        out, xyz, bad = Guarded(n, device), Guarded(n, device), _bad_flag(device)
        assert train_inputs_call(lib, device, d, shape, dev["image"], dev["noise"], V * view, view, t, out.t, dev["depth"], dev["ray_o"],
                                 dev["ray_d"], xyz.t, bad.t) == 0
        assert out.intact() and xyz.intact() and bad.intact() and int(bad.t[0]) == 0, (shape, ts)
        got = out.t.view(want_img.shape).cpu()
        assert torch.equal(got, want_img), (shape, ts, int((got != want_img).sum()))
        assert torch.equal(xyz.t.view(want_xyz.shape).cpu(), want_xyz), (shape, ts)
        assert torch.equal(dev["image"].cpu(), data["image"])              # the inputs are read, never written
        # B: the draw of the noisy views alone, without depth, in place (out_image IS image)
        img, xyz, bad = Guarded(n, device, init=data["image"]), Guarded(n, device), _bad_flag(device)
        assert train_inputs_call(lib, device, d, shape, img.t, part, (V - 1) * view, 0, t, img.t, bad=bad.t) == 0
        assert img.intact() and xyz.untouched() and bad.intact() and int(bad.t[0]) == 0, (shape, ts)
        assert torch.equal(img.t.view(want_img.shape).cpu(), want_img), (shape, ts, "in place / [B, V-1] noise")
    # C: one sample out of range (below for the first sample, above for the last): its noisy views stay as they were and so do the
    # bands, bad_t is set, every other sample and every view 0 is right, the xyz target is complete
    for b_bad, t_bad in ((0, -1), (B - 1, T)):
        ts = [417 + 100 * b for b in range(B)]
        want_img, want_xyz = expected(d, data, ts)
        ts[b_bad] = t_bad
        t = torch.tensor(ts, dtype=torch.int64, device=device)
        out, xyz, bad = Guarded(n, device), Guarded(n, device), _bad_flag(device)
        assert train_inputs_call(lib, device, d, shape, dev["image"], dev["noise"], V * view, view, t, out.t, dev["depth"], dev["ray_o"],
                                 dev["ray_d"], xyz.t, bad.t) == 0
        assert out.intact() and xyz.intact() and bad.intact(), (shape, ts)
        assert int(bad.t[0]) == (1 if V > 1 else 0), (shape, ts)           # V == 1 copies only and never looks at t
        got = out.t.view(want_img.shape).cpu()
        assert bool((got[b_bad, 1:] == FILL).all()), "the noisy views of a sample with t out of range were written"
        assert torch.equal(got[:, 0], want_img[:, 0])
        keep = [b for b in range(B) if b != b_bad]
        assert torch.equal(got[keep], want_img[keep]), (shape, ts)
        assert torch.equal(xyz.t.view(want_xyz.shape).cpu(), want_xyz), (shape, ts)
        if H * W > 1000:
            break
    # through SpacedDiffusion: the same bits, a fresh output, the caller's image untouched; q_sample on the noisy views alone
    ts = t_mixes(B)[0]
    want_img, want_xyz = expected(d, data, ts)
    t = torch.tensor(ts, dtype=torch.int64, device=device)
    x_t, gt = d.training_inputs(dev["image"], t, dev["noise"], dev["depth"], dev["ray_o"], dev["ray_d"])
    assert x_t.data_ptr() != dev["image"].data_ptr() and torch.equal(dev["image"].cpu(), data["image"])
    assert torch.equal(x_t.cpu(), want_img) and torch.equal(gt.cpu(), want_xyz) and int(d.bad_t[0]) == 0
    x_t2, none = d.training_inputs(dev["image"], t, part)
    assert none is None and torch.equal(x_t2, x_t)
    if V > 1:
        q = d.q_sample(dev["image"][:, 1:], t, noise=part)
        assert torch.equal(q.cpu(), want_img[:, 1:]), shape


def check_train_inputs_entry(lib, device):
    """Refusals: DGS_ERR_INVALID_ARGUMENT (-1) and nothing written."""
    from dgs_amd import sampler
    lib = lib or _native.lib()
    d = sampler.create_diffusion("1000", device=device, lib=lib)
    shape = (2, 2, 2, 4)
    B, V, H, W = shape
    n, view = B * V * 3 * H * W, 3 * H * W
    g = torch.Generator().manual_seed(3)
    image, noise, ray_o, ray_d = (torch.rand(B, V, 3, H, W, generator=g).to(device) for _ in range(4))
    depth = torch.rand(B, V, 1, H, W, generator=g).to(device)
    t = torch.tensor([3, 700], dtype=torch.int64, device=device)
    out, xyz, bad = Guarded(n, device), Guarded(n, device), _bad_flag(device)
    ok = dict(image=image, noise=noise, stride=V * view, offset=view, t=t, out=out.t, depth=depth, ray_o=ray_o, ray_d=ray_d, xyz=xyz.t, bad=bad.t)
    call = lambda shape_=shape, **kw: train_inputs_call(lib, device, d, shape_, **dict(ok, **kw))
    assert call((2, 2, 2, 3)) == -1                                        # H * W = 6: no whole float4 lanes
    for k in ("image", "noise", "t", "out"):
        assert call(**{k: None}) == -1, k
    assert call(tables=False) == -1
    assert call(ray_o=None) == -1 and call(ray_d=None) == -1 and call(xyz=None) == -1       # depth without both rays or without an output
    assert call((0, 2, 2, 4)) == -1 and call((2, 0, 2, 4)) == -1 and call((-1, 2, 2, 4)) == -1 and call(T_=0) == -1 and call(T_=-3) == -1
    assert call(offset=2) == -1 and call(stride=V * view + 2) == -1 and call(stride=view) == -1 and call(clean_views=3) == -1
    assert lib.dgs_train_inputs(None, _stream(device)) == -1
    assert out.untouched() and xyz.untouched() and int(bad.t[0]) == 0 and bad.intact()
    assert call() == 0                                                     # the same call with valid arguments goes through
    assert out.intact() and xyz.intact() and bool((out.t != FILL).all()) and bool((xyz.t != FILL).all())


# =====================================================================================================================================
# the trainer
# =====================================================================================================================================
def small_model(device, lib, width=256, layers=1, seed=4):
    m = dn.DGSDenoiser(dict(width=width, in_channels=9, patch_size=8, num_layers=layers), device=device, lib=lib)
    m.reset_parameters(seed=seed)
    with torch.no_grad():
        m.image_token_decoder.linear.weight.mul_(5.0)            # renders that depend visibly on the inputs
    return m.to(device).train()


def clean_batch(B, V_in, V_all, res, device, seed=1):
    """The reference's batch keys (diffusion_gs_system.py:71-102), as tests/test_ref_callers._system_case builds them; masks_input
    differ per sample (30 % and 60 % of the pixels masked out)."""
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, V_all, 3, res, res, generator=g)
    c2w = torch.tensor(np.stack([cameras.ring_cameras(V_all, phase_deg=11.0 * b) for b in range(B)]), dtype=torch.float32)
    k = torch.tensor(cameras.default_fxfycxcy(res), dtype=torch.float32).expand(B, V_all, 4).contiguous()
    thr = torch.tensor([0.3, 0.6, 0.45, 0.2][:B]).reshape(B, 1, 1, 1, 1)
    batch = {"rgbs_input": image[:, :V_in].clone(), "c2ws_input": c2w[:, :V_in].contiguous(), "fxfycxcys_input": k[:, :V_in].contiguous(),
             "depths_input": 1.5 + torch.rand(B, V_in, 1, res, res, generator=g), "c2ws": c2w, "fxfycxcys": k, "rgbs": image,
             "masks": torch.ones(B, V_all, 1, res, res), "masks_input": (torch.rand(B, V_in, 1, res, res, generator=g) > thr).float()}
    return {k_: v.to(device) for k_, v in batch.items()}


def flat_params(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()


def check_equivalence_with_step(lib, device, lambda_ssim, width=256, layers=1, res=16):
    """lambda_diffusion = 1 (and lambda_ssim on both sides when given), noise and timesteps handed in: the parameters after train_step
    equal, bit for bit, those after step() on views noised beforehand with torch ops, from the same initial state."""
    from dgs_amd import sampler
    from dgs_amd.train import DataParallelTrainer
    B, V_in, V_all = 2, 3, 4
    batch = clean_batch(B, V_in, V_all, res, device)
    keep = {k: v.clone() for k, v in batch.items()}
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(B, V_in, 3, res, res, generator=g).to(device)
    t = torch.tensor([5, 873], dtype=torch.int64, device=device)
    d = sampler.create_diffusion("1000", device=device, lib=lib)
    after = []
    for which in ("train_step", "step"):
        m = small_model(device, lib, width, layers)
        kw = dict(lambda_ssim=lambda_ssim) if (which == "step" and lambda_ssim is not None) else {}
        with DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=0.05), bucket_bytes=1 << 20, **kw) as tr:
            if which == "train_step":
                tr.configure_objective(d, dict(lambda_diffusion=1.0, lambda_ssim=lambda_ssim))
                loss = tr.train_step(batch, noise=noise, timesteps=t)
                assert tr.global_step == 1 and int(d.bad_t[0]) == 0
                logged = {k for k in tr.last_terms if k.startswith("loss_")}          # a term that is None is neither evaluated nor logged
                assert logged == ({"loss_diffusion", "loss_ssim"} if lambda_ssim is not None else {"loss_diffusion"}), logged
            else:
                a, s = d._sqrt_acp[t].reshape(B, 1, 1, 1, 1), d._sqrt_1m_acp[t].reshape(B, 1, 1, 1, 1)
                x_t = batch["rgbs_input"].clone()
                x_t[:, 1:] = a * x_t[:, 1:] + s * noise[:, 1:]
                ray_o, ray_d = m.gs_renderer.backend().rays_from_c2w(batch["c2ws_input"], batch["fxfycxcys_input"], res, res)
                loss = tr.step(dict(image=x_t, ray_o=ray_o, ray_d=ray_d, c2w=batch["c2ws"], fxfycxcy=batch["fxfycxcys"]), t, batch["rgbs"])
            after.append((flat_params(m), loss.detach().clone()))
    assert all(torch.equal(batch[k], keep[k]) for k in batch), "train_step modified the caller's batch"
    assert bool(torch.isfinite(after[0][0]).all())
    assert torch.equal(after[0][1], after[1][1]), (after[0][1], after[1][1])
    assert torch.equal(after[0][0], after[1][0]), float((after[0][0] - after[1][0]).abs().max())
    m0 = flat_params(small_model(device, lib, width, layers))
    assert not torch.equal(after[0][0], m0), "the step did not move the parameters"


def check_all_terms(lib, device, width=256, layers=1, res=16):
    """One train_step with every device term configured: finite outputs, the caller's batch unchanged, bad_t clear."""
    from dgs_amd import sampler
    from dgs_amd.train import DataParallelTrainer
    batch = clean_batch(2, 3, 4, res, device)
    keep = {k: v.clone() for k, v in batch.items()}
    d = sampler.create_diffusion("1000", device=device, lib=lib)
    m = small_model(device, lib, width, layers)
    before = flat_params(m)
    torch.manual_seed(5)
    with DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=1e-3), bucket_bytes=1 << 20) as tr:
        tr.configure_objective(d, dict(lambda_diffusion=1.0, lambda_ssim=0.2, lambda_pointsdist=[150, 1., 0., 151], lambda_xyz=0.1, lambda_lpips=None))
        loss = tr.train_step(batch)
        terms = tr.last_terms
    assert all(torch.equal(batch[k], keep[k]) for k in batch), "train_step modified the caller's batch"
    assert int(d.bad_t[0]) == 0
    for k in ("loss_diffusion", "loss_ssim", "loss_pointsdist", "loss_xyz"):
        assert terms[k].dim() == 0 and bool(torch.isfinite(terms[k])), k
    assert "loss_lpips" not in terms and "lambda_lpips" not in terms
    assert terms["lambda_pointsdist"] == 1.0 and terms["lambda_xyz"] == 0.1
    want = terms["loss_diffusion"] + 0.2 * terms["loss_ssim"] + terms["loss_pointsdist"] + 0.1 * terms["loss_xyz"]
    assert bool(torch.isfinite(loss)) and abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    now = flat_params(m)
    assert bool(torch.isfinite(now).all()) and not torch.equal(now, before)
    assert terms["timesteps"].dtype == torch.int64 and bool(((terms["timesteps"] >= 0) & (terms["timesteps"] < 1000)).all())
