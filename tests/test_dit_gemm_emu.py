"""The DiT GEMM kernels on the CPU emulator build, case by case against fp64 (gemm_util: harness, references, rules, tables).  Every case
first asserts that dgs_dit_gemm_plan reports the plan its table entry claims.

Reached here: the 128-wide two-stage kernel (BN 128 and 64, the three liveness variants of its K loop, gemv_tail_rows on and off, the
batched reduction), the ring kernel on 256 x 128 tiles and on 128 x 128 tiles with two K groups (all six epilogues on the staged strip
store; GEMV and MFMA side items with their own stores, on workgroups of their own and inside the first tile workgroups; the tail row on
the ring; no full tile row at all), the 192-wide QKV tile with the strip that straddles K | V (DGS_EMU_CUS analogues: 8 and 16 CUs),
map2d (16 and 160 CUs), split-K (DGS_SPLITK_MIN_ITEMS lowered), the pair with LayerNorm, the refusals, and ONE case each on the true
256 x 256 kernels with 8 and with 4 waves (160 tiles, K = 128).
Only the GPU reaches: everything else on 256 x 256 tiles (K = 384 and 1024, more tiles than CUs, their six epilogues and tail forms --
the emulator would need 160 tiles for each), the 192-wide tile and map2d at their production grids, split-K at a shape that
qualifies on its own, and the hardware's exp2 / rcp inside the GELU zones (the emulator's are libm's)."""
import pytest

import gemm_util as G
from emu_util import emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.mark.parametrize("case", G.EMU_CASES, ids=lambda c: c["name"])
def test_case(lib, monkeypatch, case):
    monkeypatch.setenv("DGS_EMU_CUS", str(case["cus"] or 6))
    G.run_case(lib, "cpu", case)


@pytest.mark.parametrize("case", G.EMU_SPLITK, ids=lambda c: c["name"])
def test_split_k(lib, monkeypatch, case):
    monkeypatch.setenv("DGS_SPLITK_MIN_ITEMS", "1")
    monkeypatch.setenv("DGS_EMU_CUS", "6")
    G.run_case(lib, "cpu", case)


def test_layernorm_gemm_shared_rows(lib, monkeypatch):
    monkeypatch.setenv("DGS_EMU_CUS", "6")
    G.check_layernorm_gemm(lib, "cpu")


def test_refusals(lib, monkeypatch):
    monkeypatch.setenv("DGS_EMU_CUS", "8")
    G.check_refusals(lib, "cpu")


def test_gpu_table_claims_hold_on_256_cus(lib, monkeypatch):
    """The MI355X table's plans, asked of the same host code with the emulator's chip set to 256 CUs (nothing is launched), and the
    branches of the issue's list among them: a GPU case cannot drift off its branch without this failing on a CPU-only machine too."""
    monkeypatch.setenv("DGS_EMU_CUS", "256")
    claims = [G.claim_of(G.assert_plan(lib, c)) for c in G.GPU_CASES]
    missing = [label for label, want in G.REQUIRED if not any(G.reaches(cl, want) for cl in claims)]
    assert not missing, missing
