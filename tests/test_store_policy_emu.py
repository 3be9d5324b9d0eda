"""Store policy on the CPU emulator build (store_policy_util): the emulator's memory is synchronous, so what this checks is the code
around the stores -- the wave-uniform switch in store_strip, the plan field, the LayerNorm lane-pair exchange of the through form --
not the cache behaviour.  GEMM cases: the smallest of gemm_util.EMU_CASES per (plan family x epilogue) pair that stores through, the
K | V straddle strip, valid_rows < rows_per_batch and two-row GEMV items; each under both policies, judged by gemm_util.run_case against
fp64 and bit for bit against each other."""
import ctypes

import pytest
import torch

import gemm_util as G
import rowkernel_util as R
import store_policy_util as S
from dgs_amd import _native
from emu_util import emu_lib

CASES = S.gemm_subset(G.EMU_CASES, ("128-wide", "ring 256x128", "ring 256x192", "ring 128x128"))


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture
def set_policy(lib):
    with S.policy_setter(lib) as s:
        yield s


def test_subset_reaches_the_store_paths():
    epis = {c["epi"] for c in CASES}
    assert epis >= {G.F32, G.BF16, G.GELU, G.GATE, G.QKV}, epis
    assert any(c["epi"] == G.GATE and not c["inplace"] for c in CASES) and any(c["epi"] == G.GATE and c["inplace"] for c in CASES)
    assert any("straddle" in c["name"] for c in CASES) and any(c["plan"]["tail_form"] == G.TAIL_GEMV for c in CASES)
    assert {c["plan"]["family"] for c in CASES} >= {G.FAM_128, G.FAM_RING, G.FAM_RING128}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_gemm_bit_identical_under_both_policies(lib, set_policy, monkeypatch, case):
    monkeypatch.setenv("DGS_EMU_CUS", str(case["cus"] or 6))
    S.run_gemm_both(lib, "cpu", case, set_policy, monkeypatch)


def test_rejects_values_outside_the_enum(lib, set_policy):
    for bad in (-1, 3, 100, -2 ** 31):
        assert lib.dgs_debug_store_policy(bad) == R.INVALID, bad
    for ok in (S.AUTO, S.PLAIN, S.THROUGH):
        assert lib.dgs_debug_store_policy(ok) == 0, ok


def test_a_rejected_value_leaves_the_policy(lib, set_policy, monkeypatch):
    monkeypatch.setenv("DGS_EMU_CUS", "6")
    c = next(c for c in CASES if c["epi"] == G.F32)
    set_policy(S.THROUGH)
    assert lib.dgs_debug_store_policy(7) == R.INVALID
    assert G.plan_of(lib, c)["store_policy"] == S.THROUGH
    set_policy(S.PLAIN)
    assert G.plan_of(lib, c)["store_policy"] == S.PLAIN


@pytest.mark.parametrize("width", [256, 512, 1024])
@pytest.mark.parametrize("out_f32", [False, True])
def test_layernorm_bit_identical_under_both_policies(lib, set_policy, width, out_f32):
    """rows = 5: the second workgroup is partial.  Width 256 takes the 8-byte through form, 512 and 1024 the lane-pair exchange."""
    g = torch.Generator().manual_seed(width + int(out_f32))
    rows = 5
    x = torch.randn(rows, width, generator=g) * 3 + 1
    mod = torch.randn(1, 2 * width, generator=g) * 0.3
    got = {}
    ar = R.Arena("cpu")                                     # one guarded buffer, refilled in front of each policy
    out = ar.take((rows + 3, width), torch.float32 if out_f32 else torch.bfloat16, 7.0)
    for pol in (S.PLAIN, S.THROUGH):
        set_policy(pol)
        out.fill_(7.0)
        R.call(lib, "dgs_dit_layernorm", _native.DgsDitLayerNormArgs, "cpu", rows=rows, width=width, x=x, shift=mod[:, :width], scale=mod[:, width:],
               mod_stride=2 * width, rows_per_batch=rows, eps=1e-6, out=out, out_f32=int(out_f32))
        ar.check()
        assert R.all_equal(out[rows:].float(), 7.0), "rows behind the last were written"
        got[pol] = out.clone()
    assert R.bit_equal(got[S.PLAIN], got[S.THROUGH])
    ref = torch.nn.functional.layer_norm(x.double(), (width,), eps=1e-6) * (1 + mod[:, width:].double()) + mod[:, :width].double()
    assert float((got[S.THROUGH][:rows].double() - ref).abs().max()) < (1e-4 if out_f32 else 0.05)


@pytest.mark.parametrize("width", [512, 1024])
@pytest.mark.parametrize("epi", [G.QKV, G.GELU], ids=["qkv", "gelu"])
def test_layernorm_gemm_pair_bit_identical_under_both_policies(lib, set_policy, monkeypatch, width, epi):
    monkeypatch.setenv("DGS_EMU_CUS", "6")
    S.run_pair_both(lib, "cpu", set_policy, width, epi)


def test_layernorm_gemm_pair_against_fp64_under_both_policies(lib, set_policy, monkeypatch):
    monkeypatch.setenv("DGS_EMU_CUS", "6")
    for pol in (S.PLAIN, S.THROUGH):
        set_policy(pol)
        G.check_layernorm_gemm(lib, "cpu")


@pytest.mark.parametrize("case", G.EMU_SPLITK, ids=lambda c: c["name"])
def test_split_k_plan_reports_plain_under_every_policy(lib, set_policy, monkeypatch, case):
    """The split-K partial planes never store through; the plan says PLAIN (never the zero the plan is cleared to)."""
    monkeypatch.setenv("DGS_SPLITK_MIN_ITEMS", "1")
    monkeypatch.setenv("DGS_EMU_CUS", "6")
    for pol in (S.AUTO, S.PLAIN, S.THROUGH):
        set_policy(pol)
        plan = G.plan_of(lib, case)
        assert plan["family"] == G.FAM_SPLITK and plan["store_policy"] == S.PLAIN, plan
