"""Store policy on MI355X (store_policy_util): every kernel whose bulk output store takes the policy runs under PLAIN (write-back
stores) and under THROUGH (sc1 write-through stores) on the same inputs into guarded buffers, and every byte of every output buffer
must be the same -- the policy changes how a value leaves the CU, never the value or its address.  LDS is poisoned in front of every
launch.
  GEMM       per (plan family x epilogue) pair the smallest case of gemm_util.GPU_CASES, + the strip that straddles K | V on the
             192-wide tile, + valid_rows < rows_per_batch, + two-row GEMV items; through gemm_util.run_case, so the exactness rules
             against fp64 judge the through form too; dgs_dit_gemm_plan must report the policy that ran.
  attention  heads 4, B 2: L = 34 (one query unit + 2 tail queries), 258 (one full workgroup + tail), 290 (a second, almost empty one).
  LayerNorm  widths 256 (8-byte through form) and 1024 (lane-pair exchange), 5 rows (the last workgroup is partial), bf16 / fp32,
             with and without modulation; the LayerNorm + GEMM pair (shared-rows form) at check_layernorm_gemm's shape and at width
             1024, QKV and GELU, plain against through bit for bit, + check_layernorm_gemm's fp64 rules under both.
  forward    the 64^2 step of test_smoke_c1.py: plain eager, through eager, through captured in a hipGraph and replayed three times."""
import pytest
import torch

import gemm_util as G
import rowkernel_util as R
import store_policy_util as S
from dgs_amd import _native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = S.gemm_subset(G.GPU_CASES, ("128-wide", "ring 256x256", "ring 256x192", "ring 128x128"))


@pytest.fixture(scope="module")
def ops():
    from dgs_amd.dit import DitOps
    return DitOps()


@pytest.fixture
def set_policy(ops):
    with S.policy_setter(ops.lib) as s:
        yield s


def test_subset_reaches_the_store_paths():
    fams = {name for name, fam in S.FAMILIES for c in CASES if fam(c["plan"])}
    assert fams >= {"128-wide", "ring 256x256", "ring 256x192", "ring 128x128"}, fams
    for name, fam in S.FAMILIES:
        if name in ("128-wide", "ring 256x256", "ring 128x128"):
            have = {en for en, epi in S.EPILOGUES for c in CASES if fam(c["plan"]) and epi(c)}
            assert have >= {"f32", "bf16", "gelu", "gate in place", "gate with resid"}, (name, have)
    assert any(c["epi"] == G.QKV and c["plan"]["bn"] == 192 and "straddle" in c["name"] for c in CASES)
    assert any(0 < c["valid"] < (c["rpb"] or c["M"]) for c in CASES) and any(c["plan"]["tail_form"] == G.TAIL_GEMV for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_gemm_bit_identical_under_both_policies(ops, set_policy, monkeypatch, case):
    S.run_gemm_both(ops.lib, DEV, case, set_policy, monkeypatch, before=ops.poison_lds)


@pytest.mark.parametrize("L", [34, 258, 290])
def test_attention_bit_identical_under_both_policies(ops, set_policy, L):
    heads, B, W = 4, 2, 256
    lpad = (L + 255) // 256 * 256
    g = torch.Generator().manual_seed(L)
    qk = torch.randn(B * lpad, 2 * W, generator=g).bfloat16().to(DEV)
    vt = torch.randn(B, W, lpad, generator=g).bfloat16().to(DEV)
    got = {}
    ar = R.Arena(DEV)                                       # one set of guarded buffers, refilled in front of each policy
    out = ar.take((B * lpad, W), torch.bfloat16, 7.0)
    lse = ar.take((B, heads, lpad), torch.float32, 7.0)
    for pol in (S.PLAIN, S.THROUGH):
        set_policy(pol)
        out.fill_(7.0); lse.fill_(7.0)
        ops.poison_lds()
        ops.attention(qk, vt, L, heads, lse2=lse, q_prescaled=True, out=out)
        ar.check()
        rows = out.view(B, lpad, W)
        assert R.all_equal(rows[:, L:].float(), 7.0), "rows behind the sequence were written"
        assert bool(torch.isfinite(rows[:, :L].float()).all())
        got[pol] = (out.clone(), lse.clone())
    for a, b in zip(got[S.PLAIN], got[S.THROUGH]):
        assert R.bit_equal(a, b)
    # (the values themselves are judged by the attention tests, which the plain form passes: the through form is that form bit for bit)


@pytest.mark.parametrize("width", [256, 1024])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("mod", [False, True])
def test_layernorm_bit_identical_under_both_policies(ops, set_policy, width, out_f32, mod):
    g = torch.Generator().manual_seed(width + 2 * int(out_f32) + int(mod))
    rows = 5
    x = (torch.randn(rows, width, generator=g) * 3 + 1).to(DEV)
    m = (torch.randn(1, 2 * width, generator=g) * 0.3).to(DEV)
    got = {}
    ar = R.Arena(DEV)                                       # one guarded buffer, refilled in front of each policy
    out = ar.take((rows + 3, width), torch.float32 if out_f32 else torch.bfloat16, 7.0)
    for pol in (S.PLAIN, S.THROUGH):
        set_policy(pol)
        out.fill_(7.0)
        R.call(ops.lib, "dgs_dit_layernorm", _native.DgsDitLayerNormArgs, DEV, before=ops.poison_lds, rows=rows, width=width, x=x,
               shift=m[:, :width] if mod else None, scale=m[:, width:] if mod else None, mod_stride=2 * width if mod else 0, rows_per_batch=rows, eps=1e-6,
               out=out, out_f32=int(out_f32))
        ar.check()
        assert R.all_equal(out[rows:].float(), 7.0), "rows behind the last were written"
        got[pol] = out.clone()
    assert R.bit_equal(got[S.PLAIN], got[S.THROUGH])
    ref = torch.nn.functional.layer_norm(x.double(), (width,), eps=1e-6)
    if mod:
        ref = ref * (1 + m[:, width:].double()) + m[:, :width].double()
    assert float((got[S.THROUGH][:rows].double() - ref).abs().max()) < (1e-4 if out_f32 else 0.05)


@pytest.mark.parametrize("width", [512, 1024])
@pytest.mark.parametrize("epi", [G.QKV, G.GELU], ids=["qkv", "gelu"])
def test_layernorm_gemm_pair_bit_identical_under_both_policies(ops, set_policy, width, epi):
    """The shared-rows pair (layernorm_rows_gemv_kernel) at check_layernorm_gemm's shape and at width 1024, plain against through."""
    S.run_pair_both(ops.lib, DEV, set_policy, width, epi, before=ops.poison_lds)


def test_layernorm_gemm_pair_against_fp64_under_both_policies(ops, set_policy):
    for pol in (S.PLAIN, S.THROUGH):
        set_policy(pol)
        G.check_layernorm_gemm(ops.lib, DEV, before=ops.poison_lds)


def test_whole_forward_bit_identical_eager_and_graph(ops, set_policy):
    from dgs_amd import denoiser as dn, sampler as sm
    from dgs_amd.raster import default_backend
    from oracle import dit_oracle as D
    from test_smoke_c1 import FIELDS, _case
    dev = torch.device(DEV)
    z, res, V, images, noise_T, c2w, k = _case()
    model = dn.DGSDenoiser(dict(width=1024, in_channels=9, patch_size=8, num_layers=24, ray_pe_type="relative_plk"), device=dev)
    model.load_state_dict(D.parity_state_dict(D.Cfg(), int(z["seed"])), strict=True)
    ray_o, ray_d = default_backend().rays_from_c2w(c2w.to(dev), k.to(dev), res, res)
    batch = dict(image=images.to(dev), ray_o=ray_o, ray_d=ray_d, c2w=c2w.to(dev), fxfycxcy=k.to(dev))
    diffusion = sm.create_diffusion("30", device=dev)
    t = diffusion.model_timesteps(torch.full((1,), int(z["loop_index"]), dtype=torch.int64, device=dev))

    def snapshot(rendered, gaussians):
        g = gaussians[0]
        torch.cuda.synchronize()
        return [rendered.clone()] + [x.clone() for x in (g._xyz, g._features_dc, g._scaling, g._rotation, g._opacity)]

    def same(a, b, what):
        assert len(a) == len(b) == 1 + len(FIELDS)
        for name, x, y in zip(("render",) + FIELDS, a, b):
            assert R.bit_equal(x, y), (what, name)

    with torch.no_grad():
        set_policy(S.PLAIN)
        ops.poison_lds()
        plain = snapshot(*model(batch, t))
        assert all(bool(torch.isfinite(x.float()).all()) for x in plain)
        set_policy(S.THROUGH)
        ops.poison_lds()
        same(plain, snapshot(*model(batch, t)), "through, eager")
        try:
            graphed = model.graphed(batch, t)               # captured under THROUGH: the policy rides in the captured kernel parameters
            for i in range(3):
                same(plain, snapshot(*graphed.replay()), f"through, graph replay {i}")
        finally:
            model.drop_graphs()
