"""The DiT GEMM kernels on MI355X, one dispatch branch per case against fp64 (gemm_util: harness, references, rules and the table; the
module docstring there says what is asserted).  Every case first asserts that dgs_dit_gemm_plan reports the plan its table entry
claims; test_table_reaches_every_branch asserts that the plans of the table contain every branch of gemm_util.REQUIRED.  LDS is poisoned
in front of every launch.  Measured error / bar and exception shares per case: profiles/dit_gemm_parity.txt (tools/dit_gemm_error.py)."""
import pytest
import torch

import gemm_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_and_poison():
    from dgs_amd.dit import DitOps
    ops = DitOps()
    return ops.lib, ops.poison_lds


@pytest.mark.parametrize("case", G.GPU_CASES, ids=lambda c: c["name"])
def test_case(case):
    lib, poison = _lib_and_poison()
    G.run_case(lib, DEV, case, before=poison)


def test_table_reaches_every_branch():
    lib, _ = _lib_and_poison()
    plans = [G.claim_of(G.plan_of(lib, c)) for c in G.GPU_CASES]
    missing = [label for label, want in G.REQUIRED if not any(G.reaches(p, want) for p in plans)]
    assert not missing, missing


def test_layernorm_gemm_shared_rows():
    lib, poison = _lib_and_poison()
    G.check_layernorm_gemm(lib, DEV, before=poison)


def test_refusals():
    lib, poison = _lib_and_poison()
    G.check_refusals(lib, DEV, before=poison)
    torch.cuda.empty_cache()
