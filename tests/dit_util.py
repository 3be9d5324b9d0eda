"""Shared helpers for the DiT parity tests: seeded synthetic inputs + error metrics."""
import numpy as np
import torch

from dgs_amd import cameras
from oracle import dit_oracle as D


def bf16_round_state_dict(sd):
    """The HIP path keeps GEMM weights in bf16; give the fp32 oracle the SAME (bf16-representable) weights so the parity
    tolerance only has to cover activation rounding, not weight rounding."""
    out = {}
    for k, v in sd.items():
        is_gemm_w = k.endswith("weight") and v.dim() == 2
        out[k] = v.to(torch.bfloat16).float() if is_gemm_w else v.clone()
    return out


def synth_inputs(cfg, B, V, res, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(B, V, 3, res, res, generator=g)
    c2w = torch.tensor(np.stack([cameras.ring_cameras(V, phase_deg=17.0 * b) for b in range(B)], 0))
    k = torch.tensor(cameras.default_fxfycxcy(res)).expand(B, V, 4).contiguous()
    ray_o, ray_d = D.transform_input_rays(c2w, k, res, res)
    t = torch.randint(0, 1000, (B,), generator=g)
    return images, ray_o.contiguous(), ray_d.contiguous(), t, c2w, k


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def golden_case(kind, tag="hip256"):
    """(cfg, state_dict, inputs, reference outputs) of tests/golden/dit_golden_hip256.npz for kind in {'obj','scene'}."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"dit_golden_{tag}.npz"))
    cfg = D.Cfg(width=int(z["width"]), num_layers=int(z["layers"]), scene=(kind == "scene"), range_far=50.0,
                ray_pe_type="plk" if kind == "scene" else "relative_plk",
                gaussians_sh_degree=int(z["sh_degree"]) if "sh_degree" in z.files else 0)
    sd = D.parity_state_dict(cfg, int(z["seed"]))
    t = lambda k: torch.tensor(z[kind + "_" + k])
    res = int(z["res"])
    ray_o, ray_d = D.transform_input_rays(t("in_c2w"), t("in_fxfycxcy"), res, res)
    inp = dict(images=t("in_images"), ray_o=ray_o.contiguous(), ray_d=ray_d.contiguous(), t=t("in_t"))
    ref = {k: t("out_" + k) for k in ("xyz", "features", "scaling", "rotation", "opacity", "aligned")}
    return cfg, sd, inp, ref


FIELDS = ("xyz", "features", "scaling", "rotation", "opacity")


def oracle_gradients(sd, cfg, images, ray_o, ray_d, t, wts, dev, checkpoint_blocks=False):
    """Parameter gradients of sum_k <out_k, wts_k> by torch autograd through the fp32 oracle evaluated on `dev`, ONE SAMPLE AT A
    TIME (at L = 4098 the oracle's attention matrices are ~26 GB per sample) and summed over samples in fp64.  checkpoint_blocks:
    every block under torch.utils.checkpoint (L = 16,386: 24 blocks x 2 score matrices of 17 GB would not fit; one block's do).
    Returns (outputs per field [B, ...] fp32, {state-dict key: gradient fp64})."""
    B = images.shape[0]
    leaf = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
    total = {k: torch.zeros(v.shape, dtype=torch.float64, device=dev) for k, v in leaf.items()}
    outs = {k: [] for k in FIELDS}
    for b in range(B):
        s = slice(b, b + 1)
        ref, _ = D.image_to_gaussians(leaf, cfg, images[s].to(dev), ray_o[s].to(dev), ray_d[s].to(dev), t[s].to(dev), checkpoint_blocks=checkpoint_blocks)
        sum((ref[k] * wts[k][s]).sum() for k in FIELDS).backward()
        for k, v in leaf.items():
            if v.grad is not None:
                total[k] += v.grad.double()
                v.grad = None
        for k in FIELDS:
            outs[k].append(ref[k].detach())
        del ref
    return {k: torch.cat(v, 0) for k, v in outs.items()}, total


def gradient_errors(grads, ref):
    """Per tensor: rel-L2, max |diff| / max |ref|, and for 2-D tensors the largest ROW error norm relative to the largest row norm
    (a single wrong output feature / bias row cannot hide in the tensor norm; relative to the row's OWN norm the measure is noise
    for rows of the adaLN weight gradients, which are one scalar dmod[n] times a common vector)."""
    out = {}
    for k, gv in grads.items():
        r = ref[k].double()
        g = gv.reshape(r.shape).double()
        d = g - r
        rec = {"rel_l2": float(d.norm() / r.norm().clamp_min(1e-30)), "max_abs": float(d.abs().max() / r.abs().max().clamp_min(1e-30))}
        if r.dim() == 2 and r.shape[0] > 1:
            rec["worst_row"] = float(d.norm(dim=1).max() / r.norm(dim=1).max().clamp_min(1e-30))
        out[k] = rec
    return out


# ---- whole-model cases at other learned-token (n_gaussians) and view counts ----------------------------------------------------
# (n_gaussians, B, V, res, layers, scene) at patch 8.  L = n_gaussians + V (res / 8)^2:
#   264, 520: eight tail tokens behind one / two 256-token blocks (MFMA tail items in the GEMMs, one attention-backward workgroup per
#             tail token: 9 / 10 partial rows of the qkv bias gradient against 4 / 6 that lpad / 128 gives);
#   260 x 2 samples, 257 x 3, 259 (scene): tails of 4, 1 (one-row GEMV) and 3 tokens;  322, 194: no learned-token tail rule applies
#   (five and three views: the generic ragged last tile).
# The one-layer cases stay at one layer: the slab carved behind the qkv bias partials (the adaLN Linear's, sized by the layer count) is
# then smaller than the rows a too-small carve would miss, so those rows leave the workspace instead of landing in a slab that is
# rewritten before it is read.
LEARNED_TOKEN_CASES = [(8, 1, 4, 64, 1, False), (8, 1, 2, 128, 1, False), (4, 2, 4, 64, 1, False), (1, 3, 4, 64, 2, False),
                       (3, 1, 4, 64, 2, True), (2, 1, 5, 64, 2, False), (2, 1, 3, 64, 2, False)]
# (n_gaussians, V) of the forward-only cases at res 64, one sample: L = 257, 259, 264, 268 (outside every tail rule), 194
LEARNED_TOKEN_FORWARD_CASES = [(1, 4), (3, 4), (8, 4), (12, 4), (2, 3)]

GUARD_BYTE, GUARD_BYTES = 0xA5, 1 << 16


def learned_token_cfg(ng, layers, scene, width):
    return D.Cfg(width=width, num_layers=layers, n_gaussians=ng, scene=scene, ray_pe_type="plk" if scene else "relative_plk",
                 range_far=50.0)


def learned_token_engine(cfg, sd, device, lib=None):
    from dgs_amd.dit import DitEngine
    return DitEngine(sd, width=cfg.width, num_layers=cfg.num_layers, n_gaussians=cfg.n_gaussians, ray_pe_type=cfg.ray_pe_type,
                     scene=cfg.scene, range_near=cfg.range_near, range_far=cfg.range_far, device=device, lib=lib)


def guard_arena(eng, ar, which):
    """Swap the arena's `which` ('bws': backward workspace, 'saved': activation arena) for a view of a larger buffer of the same device
    and dtype whose tail (64 KiB behind the view) is filled with 0xA5.  The view keeps the contents and numel() -- the byte counts the
    engine hands to the library do not change -- so a kernel that writes past the size the library itself asked for lands in memory
    this test owns.  Returns a checker that asserts the tail is untouched (and synchronises first on a GPU)."""
    old = ar[which]
    n = old.numel()
    big = torch.empty(n + GUARD_BYTES, dtype=old.dtype, device=old.device)
    big[:n].copy_(old)
    big[n:].fill_(GUARD_BYTE)
    ar[which] = big[:n]
    tr = eng._train
    if tr.get("current") is ar:      # the engine's mirrors of the most recently used arena
        tr[which] = ar[which]

    def check():
        if big.device.type == "cuda":
            torch.cuda.synchronize(big.device)
        dirty = int((big[n:] != GUARD_BYTE).sum())
        assert dirty == 0, f"{dirty} bytes written past the end of the {n}-byte '{which}' arena"
    return check


def guarded_forward_train(eng, images, ray_o, ray_d, t, recompute=False):
    """eng.forward_train with both arenas of the pass under guard_arena.  Returns (outputs, aligned, arena, check): pass the arena to
    eng.backward(..., arena=arena), then call check() -- it is also run on the activation arena right after the forward."""
    B, V, _, H, W = images.shape
    ar = eng._arena(B, V, H, W, bool(recompute), False)
    checks = [guard_arena(eng, ar, "saved"), guard_arena(eng, ar, "bws")]
    out, aligned = eng.forward_train(images, ray_o, ray_d, t, recompute=recompute)
    assert eng._train["current"] is ar
    checks[0]()

    def check():
        for c in checks:
            c()
    return out, aligned, ar, check
