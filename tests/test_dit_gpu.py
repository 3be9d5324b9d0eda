"""Parity tests proper for the denoiser half: gfx950 kernels through the C ABI vs (a) golden vectors produced by the
reference's own code, (b) the fp32 oracle on CPU at sizes it finishes in seconds, (c) at BASELINE.json's full size
(256^2, L = 4098, width 1024, 24 blocks) the same fp32 oracle evaluated with torch on the GPU as the checker.
Tolerances (bf16 operands, fp32 accumulate / residual / statistics): rel-L2 <= 1e-2 on tokens, <= 2e-2 on Gaussian
parameters."""
import pytest
import torch
import torch.nn.functional as F

from dgs_amd import _native
from dit_util import LEARNED_TOKEN_FORWARD_CASES, golden_case, rel_l2, synth_inputs
from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def poisoned_lds():
    """Every test starts from LDS full of NaN patterns: the GEMM / attention kernels read fragments that LDS-DMAs deliver
    asynchronously, and a read that overtook its DMA would otherwise find the previous test's -- often identical -- data."""
    from dgs_amd.dit import DitOps
    DitOps().poison_lds()
    yield
FIELDS = ("xyz", "features", "scaling", "rotation", "opacity")
DEV = "cuda:0"


class _Poisoned:
    """DitOps whose every kernel call starts from NaN-filled LDS (poisoned_lds above covers only a test's first launch)."""

    def __init__(self, ops):
        self._ops = ops

    def __getattr__(self, name):
        fn = getattr(self._ops, name)

        def call(*a, **k):
            self._ops.poison_lds()
            return fn(*a, **k)
        return call


def _ops():
    from dgs_amd.dit import DitOps
    return _Poisoned(DitOps())


def _bf(t):
    return t.to(torch.bfloat16)


def test_qkv_gemm_on_192_wide_tiles_at_the_model_shape():
    """QKV at one sample (4,352 padded / 4,098 live rows, N = 3,072): 16 x 16 tiles of 256 x 192, one per CU (256-wide tiles are 192).
    Against fp32 math and against the 128-wide kernel family (same slab order: equal up to the output rounding), q pre-scaled, V only
    transposed, the learned tokens' two rows included."""
    from dgs_amd.dit import DitOps
    ops = DitOps()
    g = torch.Generator(device=DEV).manual_seed(3072)
    M, N, K, L, Wd = 4352, 3072, 1024, 4098, 1024
    A = _bf(torch.randn(M, K, generator=g, device=DEV))
    W = _bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
    bias = torch.randn(N, generator=g, device=DEV)
    ref = A.float() @ W.float().t() + bias
    ops.poison_lds()
    qk, vt = ops.gemm(A, W, bias, _native.EPI_QKV, rows_per_batch=M, valid_rows=L, q_scale=0.18)
    assert ops.last_gemm_sliced_tile == 192
    qk2, vt2 = ops.gemm(A, W, bias, _native.EPI_QKV, rows_per_batch=M, valid_rows=L, q_scale=0.18, algo=_native.GEMM_SIMPLE128)
    assert ops.last_gemm_sliced_tile == 0
    assert rel_l2(qk[:L, :Wd].float(), 0.18 * ref[:L, :Wd]) < 4e-3 and rel_l2(qk[:L, Wd:].float(), ref[:L, Wd:2 * Wd]) < 4e-3
    assert rel_l2(vt[0, :, :L].float(), ref[:L, 2 * Wd:].t()) < 4e-3
    assert bool((qk[L:] == 0).all()) and bool((vt[0, :, L:] == 0).all())          # padding: never written
    assert float((qk[:L].float() - qk2[:L].float()).abs().max()) <= 2e-2 * float(qk2[:L].float().abs().max())
    assert float((vt[0, :, :L].float() - vt2[0, :, :L].float()).abs().max()) <= 2e-2 * float(vt2.float().abs().max())


@pytest.mark.parametrize("width,N,qkv,B", [(1024, 3072, True, 1), (1024, 4096, False, 1), (1024, 3072, True, 4), (1024, 4096, False, 2)])
def test_layernorm_gemm_pair_at_the_model_shape(width, N, qkv, B):
    """The DiT's LayerNorm -> QKV / fc1 pairs at L = 4,098 (lpad 4,352) as dgs_dit_forward launches them (AUTO kernel choice): the learned
    tokens' rows produced inside the LayerNorm launch, every output bit-identical to the two plain launches."""
    from dgs_amd.dit import DitOps
    from test_dit_kernels_emu import _check_layernorm_gemm_pair
    ops = DitOps()
    ops.poison_lds()
    _check_layernorm_gemm_pair(ops, DEV, width, N, qkv, valids=(4098, 4097), B=B, rpb=4352, algo=_native.GEMM_AUTO)


@pytest.mark.parametrize("N", [768, 25344])
def test_gemm_sliced_single_block_mfma_items(N):
    """The ring kernel's single-block MFMA side items through every epilogue that reaches their store: on 128-wide tiles (N = 768), and
    on 256-wide tiles, 8 and 4 waves (N = 25,344: 2 x 99 tiles of 256 x 256 fill the chip, and 2 x 132 of 256 x 192 do not fit it)."""
    from dgs_amd.dit import DitOps
    from test_dit_kernels_emu import _check_single_block_mfma_items
    _check_single_block_mfma_items(DitOps(), DEV, N)


# What dgs_dit_gemm_plan says each `algo` iteration of test_gemm_production_shapes runs (family, tile width, waves): M = 4224 is no
# multiple of 256 and K = 576 none of 128, so SLICED / QUAD fall back to the 128-wide kernel there; (256, 896, 1024) runs the ring's
# 256 x 128 tile (QUAD has no 4-wave form of it); M = 4352 is the eligible shape: 17 x 12 tiles of 256 x 256, 8 and 4 waves.
_SIMPLE128, _RING = _native.GEMM_FAMILY_SIMPLE128, _native.GEMM_FAMILY_RING256
_PRODUCTION_PLANS = {(4224, 3072, 1024): {1: (_SIMPLE128, 128, 4), 4: (_SIMPLE128, 128, 4), 5: (_SIMPLE128, 128, 4)},
                     (4224, 1024, 4096): {1: (_SIMPLE128, 64, 4), 4: (_SIMPLE128, 64, 4), 5: (_SIMPLE128, 64, 4)},
                     (256, 896, 1024): {1: (_SIMPLE128, 64, 4), 4: (_RING, 128, 8), 5: (_RING, 128, 8)},
                     (4224, 1024, 576): {1: (_SIMPLE128, 64, 4), 4: (_SIMPLE128, 64, 4), 5: (_SIMPLE128, 64, 4)},
                     (4352, 3072, 1024): {1: (_SIMPLE128, 128, 4), 4: (_RING, 256, 8), 5: (_RING, 256, 4)}}


def _plan_key(plan):
    return plan["family"], plan["bn"], plan["waves"]


@pytest.mark.parametrize("M,N,K", [(4224, 3072, 1024), (4224, 1024, 4096), (256, 896, 1024), (4224, 1024, 576), (4352, 3072, 1024)])
def test_gemm_production_shapes(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    A = _bf(torch.randn(M, K, generator=g, device=DEV))
    W = _bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
    bias = torch.randn(N, generator=g, device=DEV)
    ref = A.float() @ W.float().t() + bias
    ops = _ops()
    assert rel_l2(ops.gemm(A, W, bias, _native.EPI_F32), ref) < 1e-5
    for algo in (_native.GEMM_SIMPLE128, _native.GEMM_SLICED, _native.GEMM_QUAD):   # every kernel family (ineligible shapes fall back)
        for epi in (_native.EPI_F32, _native.EPI_GELU_BF16):
            assert _plan_key(ops.gemm_plan(A, W, bias, epi, algo=algo)) == _PRODUCTION_PLANS[M, N, K][algo], (algo, epi)
        assert rel_l2(ops.gemm(A, W, bias, _native.EPI_F32, algo=algo), ref) < 1e-5, algo
        assert rel_l2(ops.gemm(A, W, bias, _native.EPI_GELU_BF16, algo=algo).float(), F.gelu(ref, approximate="tanh")) < 4e-3, algo
    assert rel_l2(ops.gemm(A, W, bias, _native.EPI_BF16).float(), ref) < 4e-3
    assert rel_l2(ops.gemm(A, W, bias, _native.EPI_GELU_BF16).float(), F.gelu(ref, approximate="tanh")) < 4e-3
    rows = 128 if M % 384 else 384
    x0 = torch.randn(M, N, generator=g, device=DEV)
    gate = torch.randn(M // rows, N, generator=g, device=DEV)
    x = x0.clone()
    ops.gemm(A, W, bias, _native.EPI_GATE_RESIDUAL, out=x, gate=gate, rows_per_batch=rows)
    assert rel_l2(x, x0 + gate.repeat_interleave(rows, 0) * ref) < 1e-5
    if N % 384 == 0:
        qk, vt = ops.gemm(A, W, bias, _native.EPI_QKV, rows_per_batch=M)
        Wd = N // 3
        assert rel_l2(qk.float(), ref[:, :2 * Wd]) < 4e-3
        assert rel_l2(vt.float()[0], ref[:, 2 * Wd:].t()) < 4e-3


@pytest.mark.parametrize("name,N,K,epi", [("qkv", 3072, 1024, "QKV"), ("proj", 1024, 1024, "GATE_RESIDUAL"),
                                          ("fc1", 4096, 1024, "GELU_BF16"), ("fc2", 1024, 4096, "GATE_RESIDUAL")])
def test_block_gemms_at_the_shipped_shape_incl_learned_token_rows(name, N, K, epi):
    """One sample at 256^2: 4,352 padded rows, 4,098 valid -- 32 full 128-row tiles plus the two learned-token rows, which every
    kernel family treats specially (GEMV items behind the tile grid / side jobs of the first workgroups / workgroups of their own on
    idle CUs).  Checked on the full tiles AND on those two rows separately: two wrong rows of 4,098 would hide in a tensor-wide norm."""
    M, L = 4352, 4098
    g = torch.Generator(device=DEV).manual_seed(len(name) + N + K)
    A = _bf(torch.randn(M, K, generator=g, device=DEV))
    W = _bf(torch.randn(N, K, generator=g, device=DEV) * 0.05)
    bias = torch.randn(N, generator=g, device=DEV)
    ref = A.float() @ W.float().t() + bias
    ops = _ops()
    e = getattr(_native, "EPI_" + epi)
    for algo in (_native.GEMM_AUTO, _native.GEMM_SIMPLE128, _native.GEMM_SLICED, _native.GEMM_SLICED128):
        kw = dict(rows_per_batch=M, valid_rows=L, algo=algo)
        if epi == "GATE_RESIDUAL":
            x0 = torch.randn(M, N, generator=g, device=DEV)
            gate = torch.randn(1, N, generator=g, device=DEV)
            x = x0.clone()
            ops.gemm(A, W, bias, e, out=x, gate=gate, **kw)
            got, want, tol = x, x0 + gate * ref, 1e-5
        elif epi == "GELU_BF16":
            got, want, tol = ops.gemm(A, W, bias, e, **kw).float(), F.gelu(ref, approximate="tanh"), 4e-3
        else:
            qk, vt = ops.gemm(A, W, bias, e, **kw)
            Wd = N // 3
            got = torch.cat([qk.float()[:, :2 * Wd], vt.float()[0].t()], dim=1)
            want, tol = ref, 4e-3
        assert rel_l2(got[:L - 2], want[:L - 2]) < tol, (name, algo, "full tiles")
        assert rel_l2(got[L - 2:L], want[L - 2:L]) < tol, (name, algo, "learned-token rows")


@pytest.mark.parametrize("algo", [0, _native.GEMM_SLICED, _native.GEMM_QUAD])
def test_gemm_training_epilogues_production_shapes(algo):
    """fc1 forward (GELU + saved pre-activation + transposed copy) and the fc2 input gradient (dGELU + transposed copy) at the
    4-view token count, 2 samples with padding rows: values vs fp32 torch, transposed copies bit-equal to the row-major ones.
    4,224 rows per sample are no multiple of 256: every `algo` runs the 128-wide kernel here (asserted)."""
    _training_epilogues(algo, 4224, (_SIMPLE128, 128, 4))


@pytest.mark.parametrize("algo", [0, _native.GEMM_SLICED, _native.GEMM_QUAD])
def test_gemm_training_epilogues_ring_eligible_shape(algo):
    """The same with 4,352 rows per sample (the padding dgs_dit_lpad gives): 2 x 16 x 16 full tiles of 256 x 256 on the ring kernel, 8 waves
    (AUTO: more than 8,192 rows; SLICED) or 4 (QUAD), the learned tokens' rows as GEMV side items."""
    _training_epilogues(algo, 4352, (_RING, 256, 4 if algo == _native.GEMM_QUAD else 8))


def _training_epilogues(algo, rows, plan_key):
    B, L, W = 2, 4098, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    ops = _ops()
    x = _bf(torch.randn(B * rows, W, generator=g, device=DEV))
    w1 = _bf(torch.randn(4 * W, W, generator=g, device=DEV) * 0.03)
    b1 = torch.randn(4 * W, generator=g, device=DEV) * 0.1
    u_ref = x.float() @ w1.float().t() + b1
    live = (torch.arange(B * rows, device=DEV) % rows) < L
    tr = lambda t, n: t.reshape(B, rows, n).transpose(1, 2)
    vt = torch.zeros(B, 4 * W, rows, dtype=torch.bfloat16, device=DEV)
    aux = torch.zeros(B * rows, 4 * W, dtype=torch.bfloat16, device=DEV)
    assert _plan_key(ops.gemm_plan(x, w1, b1, _native.EPI_GELU_BF16, rows_per_batch=rows, valid_rows=L, vt=vt, aux=aux, algo=algo)) == plan_key
    out = ops.gemm(x, w1, b1, _native.EPI_GELU_BF16, rows_per_batch=rows, valid_rows=L, vt=vt, aux=aux, algo=algo)
    assert rel_l2(aux.float()[live], u_ref[live]) < 4e-3
    assert rel_l2(out.float()[live], F.gelu(u_ref, approximate="tanh")[live]) < 4e-3
    assert torch.equal(vt[:, :, :L], tr(out, 4 * W)[:, :, :L])
    dy = _bf(torch.randn(B * rows, W, generator=g, device=DEV))
    w2t = _bf(torch.randn(4 * W, W, generator=g, device=DEV) * 0.03)          # K-contiguous copy of fc2.weight
    uu = aux.float().requires_grad_(True)
    F.gelu(uu, approximate="tanh").sum().backward()
    assert _plan_key(ops.gemm_plan(dy, w2t, None, _native.EPI_DGELU_BF16, rows_per_batch=rows, valid_rows=L, vt=vt, aux=aux, algo=algo)) == plan_key
    du = ops.gemm(dy, w2t, None, _native.EPI_DGELU_BF16, rows_per_batch=rows, valid_rows=L, vt=vt, aux=aux, algo=algo)
    assert rel_l2(du.float()[live], ((dy.float() @ w2t.float().t()) * uu.grad)[live]) < 5e-3
    assert torch.equal(vt[:, :, :L], tr(du, 4 * W)[:, :, :L])


@pytest.mark.parametrize("prescaled", [True, False])
@pytest.mark.parametrize("L,B", [(4098, 1), (258, 2), (1026, 1), (16386, 1), (290, 1), (18, 2), (4130, 1)])
def test_attention_production_shapes(L, B, prescaled):
    """prescaled: q arrives as bf16(scale * log2(e) * q) like from the QKV GEMM epilogue (one rounding, the path the
    denoiser uses); otherwise the kernel scales the bf16 queries itself (a second bf16 rounding: looser max-abs bound).
    L = 16386 is the 512^2 configuration (BASELINE configs[4]); 290 / 4130 have a tail tile behind a number of full tiles
    that is not a multiple of the 8 waves, 18 has no full tile at all (the tail-record hand-off of every wave shape)."""
    heads = 16
    lpad = (L + 127) // 128 * 128
    g = torch.Generator(device=DEV).manual_seed(L)
    q, k, v = (torch.randn(B, heads, lpad, 64, generator=g, device=DEV) for _ in range(3))
    q[0, 3, 5] *= 8.0   # force large running-max jumps (rule 26: the rescale branch must be exercised)
    k[0, 3, L - 1] *= 8.0
    c = 0.125 * 1.4426950408889634
    qb, kb, vb = (_bf(q * c) if prescaled else _bf(q)), _bf(k), _bf(v)
    qk = torch.cat([qb.permute(0, 2, 1, 3).reshape(B * lpad, heads * 64), kb.permute(0, 2, 1, 3).reshape(B * lpad, heads * 64)], 1).contiguous()
    vt = vb.permute(0, 1, 3, 2).reshape(B, heads * 64, lpad).contiguous()
    out = _ops().attention(qk, vt, L, heads, q_prescaled=prescaled).float().reshape(B, lpad, heads, 64).permute(0, 2, 1, 3)[:, :, :L]
    num = den = 0.0
    worst = 0.0
    for b in range(B):
        for h in range(heads):     # one head at a time: the fp64 score matrix of L = 16386 is 2 GB
            s = (qb[b, h, :L].double() @ kb[b, h, :L].double().t()) * (0.6931471805599453 if prescaled else 0.125)
            ref = s.softmax(-1) @ vb[b, h, :L].double()
            d = out[b, h].double() - ref
            num += float((d * d).sum()); den += float((ref * ref).sum()); worst = max(worst, float(d.abs().max()))
    assert (num / den) ** 0.5 < 6e-3
    assert worst < (3e-2 if prescaled else 4e-2)


def test_reserved_tail_mode_is_rejected():
    """`DgsDitAttentionArgs.tail_mode` is reserved (rounds 4-5 ran the L % 32 tail queries as a launch of their own behind it: measured,
    lost twice, kept as tools/next/tail_chain_experiment.patch): anything but 0 is an invalid argument."""
    L, B, heads = 258, 1, 16
    lpad = 384
    qk = torch.zeros(B * lpad, 2 * heads * 64, dtype=torch.bfloat16, device=DEV)
    vt = torch.zeros(B, heads * 64, lpad, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="status"):
        _ops().attention(qk, vt, L, heads, q_prescaled=True, tail_mode=1)



@pytest.mark.parametrize("kind", ["obj", "scene"])
def test_forward_matches_reference_golden(kind):
    from dgs_amd.dit import DitEngine
    cfg, sd, inp, ref = golden_case(kind)
    eng = DitEngine(sd, width=cfg.width, num_layers=cfg.num_layers, ray_pe_type=cfg.ray_pe_type, scene=cfg.scene,
                    range_near=cfg.range_near, range_far=cfg.range_far, device=DEV)
    out, aligned = eng.image_to_gaussians(inp["images"], inp["ray_o"], inp["ray_d"], inp["t"])
    for k in FIELDS:
        assert rel_l2(out[k].cpu(), ref[k]) < 2e-2, (k, rel_l2(out[k].cpu(), ref[k]))
    assert rel_l2(aligned.cpu(), ref["aligned"]) < 2e-2


def test_forward_sh_degree_1_matches_reference_golden_and_renders():
    """gaussians_sh_degree = 1 on the MI355X: the engine against the golden vectors of the reference's own denoiser (23 Gaussian channels,
    features [b, P, 4, 3]); then the whole DGSDenoiser.forward with that degree -- the rasterizer evaluates the degree-1 harmonics of
    the denoiser's own features -- against the drop-in binding's render of the same Gaussians."""
    from dgs_amd import denoiser as dn
    from dgs_amd.dit import DitEngine
    cfg, sd, inp, ref = golden_case("obj", tag="hip256_sh1")
    eng = DitEngine(sd, width=cfg.width, num_layers=cfg.num_layers, ray_pe_type=cfg.ray_pe_type, gaussians_sh_degree=1, device=DEV)
    out, aligned = eng.image_to_gaussians(inp["images"], inp["ray_o"], inp["ray_d"], inp["t"])
    for k in FIELDS:
        assert out[k].shape == ref[k].shape, k
        assert rel_l2(out[k].cpu(), ref[k]) < 2e-2, (k, rel_l2(out[k].cpu(), ref[k]))
    m = dn.DGSDenoiser(dict(width=256, in_channels=9, patch_size=8, num_layers=2, gaussians_sh_degree=1), device=DEV)
    m.reset_parameters(seed=4)
    images, ray_o, ray_d, t, c2w, k = synth_inputs(D.Cfg(width=256, num_layers=2, gaussians_sh_degree=1), 1, 4, 64, seed=6)
    batch = {a: b.to(DEV) for a, b in dict(image=images, ray_o=ray_o, ray_d=ray_d, c2w=c2w, fxfycxcy=k).items()}
    with torch.no_grad():                      # inference: the training calls take degree 0 (NotImplementedError otherwise)
        rendered, gaussians = m(batch, t.to(DEV))
    assert rendered.shape == (1, 4, 3, 64, 64) and torch.isfinite(rendered).all() and float(rendered.std()) > 1e-3
    with pytest.raises(NotImplementedError):
        m(batch, t.to(DEV))
    import diff_gaussian_rasterization as dgr
    from dgs_amd.raster import default_backend
    g = gaussians[0]
    assert g.get_features.shape[-2:] == (4, 3)
    view, proj, campos, tanfov = default_backend().cameras_from_c2w(batch["c2w"], batch["fxfycxcy"], 64, 64)
    rs = dgr.GaussianRasterizationSettings(64, 64, float(tanfov[2, 0]), float(tanfov[2, 1]), torch.ones(3, device=DEV), 1.0,
                                           view[2], proj[2], 1, campos[2], False, False)
    color, _ = dgr.GaussianRasterizer(rs)(g.get_xyz, torch.zeros_like(g.get_xyz), g.get_opacity, shs=g.get_features,
                                          scales=g.get_scaling, rotations=g.get_rotation)
    assert float(((color.clamp(0, 1) - rendered[0, 2].clamp(0, 1)) ** 2).mean()) < 1e-7


@pytest.mark.parametrize("kind", ["obj"])
def test_forward_matches_reference_golden_258_tokens(kind):
    """A fixture from the reference's own denoiser code at 258 tokens (res 64, 4 views): multi-tile attention, the key
    ring and the learned-token tail merge are pinned to the reference directly, not through the oracle."""
    from dgs_amd.dit import DitEngine
    cfg, sd, inp, ref = golden_case(kind, tag="hip256_l258")
    eng = DitEngine(sd, width=cfg.width, num_layers=cfg.num_layers, ray_pe_type=cfg.ray_pe_type, scene=cfg.scene,
                    range_near=cfg.range_near, range_far=cfg.range_far, device=DEV)
    out, aligned = eng.image_to_gaussians(inp["images"], inp["ray_o"], inp["ray_d"], inp["t"])
    for k in FIELDS:
        assert rel_l2(out[k].cpu(), ref[k]) < 2e-2, (k, rel_l2(out[k].cpu(), ref[k]))
    assert rel_l2(aligned.cpu(), ref["aligned"]) < 2e-2


def _full_model_case(res, B, oracle_device, scene=False):
    from dgs_amd.dit import DitEngine
    cfg = D.Cfg(scene=scene, ray_pe_type="plk" if scene else "relative_plk")   # width 1024, 24 blocks, patch 8: the shipped models
    sd = D.parity_state_dict(cfg, seed=11)
    images, ray_o, ray_d, t, _, _ = synth_inputs(cfg, B, 4, res, seed=3)
    eng = DitEngine(sd, device=DEV, scene=cfg.scene, ray_pe_type=cfg.ray_pe_type, range_near=cfg.range_near, range_far=cfg.range_far)
    out, aligned = eng.image_to_gaussians(images, ray_o, ray_d, t, return_tokens=True)
    torch.cuda.synchronize()
    sd_o = {k: v.to(oracle_device) for k, v in sd.items()}
    with torch.no_grad():
        ref, ref_aligned = D.image_to_gaussians(sd_o, cfg, images.to(oracle_device), ray_o.to(oracle_device),
                                                ray_d.to(oracle_device), t.to(oracle_device), return_tokens=True)
    assert rel_l2(out["tokens"].cpu(), ref["tokens"].cpu()) < 1e-2, rel_l2(out["tokens"].cpu(), ref["tokens"].cpu())
    for k in FIELDS:
        assert rel_l2(out[k].cpu(), ref[k].cpu()) < 2e-2, (k, rel_l2(out[k].cpu(), ref[k].cpu()))
    assert rel_l2(aligned.cpu(), ref_aligned.cpu()) < 2e-2
    assert all(torch.isfinite(out[k]).all() for k in FIELDS)


def test_full_model_64_vs_cpu_oracle():
    _full_model_case(64, 2, "cpu")


def test_full_model_256_vs_fp32_oracle_on_gpu():
    _full_model_case(256, 1, DEV)


def test_full_model_512_vs_fp32_oracle_on_gpu():
    """BASELINE configs[4] (scene model, 512^2): L = 16,386 tokens, P = 1,048,578 Gaussians, all 24 blocks."""
    _full_model_case(512, 1, DEV, scene=True)


@pytest.mark.parametrize("ng,V", LEARNED_TOKEN_FORWARD_CASES)
def test_forward_at_other_learned_token_and_view_counts(ng, V):
    """The inference forward at width 1024 (the shipped GEMM dispatch: GEMV rows need K >= 512), two blocks, at token counts other
    than 256 k + 2: one learned token (one-row GEMV), 3 and 8 (MFMA tail items, the LayerNorm+GEMM pair as two launches), 12 (L = 268,
    outside every tail rule) and three views (L = 194).  _full_model_case's bars; the learned tokens' own rows also on their own."""
    import os
    from dit_util import learned_token_cfg, learned_token_engine
    cfg = learned_token_cfg(ng, 2, False, width=1024)
    sd = D.parity_state_dict(cfg, seed=11)
    B, res = 1, 64
    images, ray_o, ray_d, t, _, _ = synth_inputs(cfg, B, V, res, seed=3)
    eng = learned_token_engine(cfg, sd, DEV)
    out, aligned = eng.image_to_gaussians(images, ray_o, ray_d, t, return_tokens=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref, ref_aligned = D.image_to_gaussians({k: v.to(DEV) for k, v in sd.items()}, cfg, images.to(DEV), ray_o.to(DEV), ray_d.to(DEV),
                                                t.to(DEV), return_tokens=True)
    cat = lambda o: torch.cat([o[k][:, :ng].reshape(B, ng, -1) for k in FIELDS], -1)
    errs = {"tokens": rel_l2(out["tokens"], ref["tokens"]), "learned_token_rows": rel_l2(out["tokens"][:, :ng], ref["tokens"][:, :ng]),
            "learned_token_gaussians": rel_l2(cat(out), cat(ref)), "aligned": rel_l2(aligned, ref_aligned)}
    errs.update({k: rel_l2(out[k], ref[k]) for k in FIELDS})
    line = f"forward n_gaussians={ng} V={V} res={res} L={eng.num_tokens(V, res, res)}: " + " ".join(f"{k}={e:.2e}" for k, e in errs.items())
    print(line)
    if os.environ.get("DGS_LEARNED_TOKEN_PARITY_DUMP"):
        with open(os.environ["DGS_LEARNED_TOKEN_PARITY_DUMP"], "a") as f:
            f.write(line + "\n")
    assert out["tokens"].shape == ref["tokens"].shape
    assert errs["tokens"] < 1e-2 and errs["learned_token_rows"] < 1e-2, errs
    for k in FIELDS:
        assert out[k].shape == ref[k].shape, k
        assert errs[k] < 2e-2, (k, errs)
    assert errs["learned_token_gaussians"] < 2e-2 and errs["aligned"] < 2e-2, errs
    assert all(torch.isfinite(out[k]).all() for k in FIELDS)


def test_denoiser_forward_end_to_end_256():
    """DGSDenoiser.forward (DiT step + 4 rasterizations at 256^2): shapes, finiteness, and the render of the HIP path's
    own Gaussians re-rendered per view through the drop-in `diff_gaussian_rasterization` binding (same kernels,
    reference call convention: activated parameters, one view per call) must agree bit for bit with the batched path
    up to the fused-activation rounding."""
    from dgs_amd import denoiser as dn
    cfg = D.Cfg()
    m = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=24), device=DEV)
    m.reset_parameters(seed=2)
    images, ray_o, ray_d, t, c2w, k = synth_inputs(cfg, 1, 4, 256, seed=5)
    batch = {a: b.to(DEV) for a, b in dict(image=images, ray_o=ray_o, ray_d=ray_d, c2w=c2w, fxfycxcy=k).items()}
    rendered, gaussians = m(batch, t.to(DEV))
    assert rendered.shape == (1, 4, 3, 256, 256) and torch.isfinite(rendered).all()
    assert float(rendered.min()) >= 0.0 and float(rendered.std()) > 1e-3
    import diff_gaussian_rasterization as dgr
    g = gaussians[0]
    from dgs_amd.raster import default_backend
    view, proj, campos, tanfov = default_backend().cameras_from_c2w(batch["c2w"], batch["fxfycxcy"], 256, 256)
    rs = dgr.GaussianRasterizationSettings(256, 256, float(tanfov[1, 0]), float(tanfov[1, 1]), torch.ones(3, device=DEV), 1.0,
                                           view[1], proj[1], 0, campos[1], False, False)
    color, radii = dgr.GaussianRasterizer(rs)(g.get_xyz, torch.zeros_like(g.get_xyz), g.get_opacity, shs=g.get_features,
                                              scales=g.get_scaling, rotations=g.get_rotation)
    mse = float(((color.clamp(0, 1) - rendered[0, 1].clamp(0, 1)) ** 2).mean())
    assert mse < 1e-7, mse   # > 70 dB
