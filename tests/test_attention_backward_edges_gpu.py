"""Attention backward on MI355X at sequence-length and batch edges (attn_bwd_util.CASES: B up to 4, 1 / 2 / 8 tail tokens, a rest of 9
and 34 rows, L below one block and below the ring depth, L == lpad, lpad above the minimum, a last block that reaches past lpad, both
workgroup numberings), where the two production-length tests run B = 1 and L % 256 = 2 only.  Per case (attn_bwd_util.check_case):

  forward      o within 6e-3 rel-L2 of fp64; lse2 of every valid query within 2^-8 max_k sum_d |c q_d k_d| + 1e-4
  backward     twice, outputs between guard bands (dqkv valid rows pre-filled with 7.0, D with 3.0): bit-equal, guards untouched, padding
               rows exactly zero, valid rows finite
  accuracy     normalised RMS error per (tensor, sample, head) slice, per 64-row tile and per row <= 3 x the worst error, at that
               granularity in this case, of an fp64 restatement with the kernel's five bf16 roundings (+ 1e-6): a dropped 64-row tile
               moves a row by ~1 / sqrt(tiles) (>= 0.12 at 65 tiles), a wrong head or sample by ~1.4, the bars are ~1e-2 (slice, tile) and
               2.5 - 4.5e-2 (row); the project's tensor-wide 1.5e-2 as well
  D            -sum_d o dO in fp64 from the same bf16 o and dO, within 1e-5 sum_d |o dO|
  by-products  _check_attention_backward_byproducts through a guarded launch; every bias_part slot against the column sum of its own
               rows; a tail token's slot rounds to its dqkv row bit for bit
Measured: profiles/attn_bwd_edges_parity.txt (tools/attn_bwd_edge_error.py): kernel / model at most 1.31 (L = 3: the forward's o and lse2 carry
more than the model's one rounding; with them put into the model it reproduces the kernel bit for bit), 0.67 - 1.07 elsewhere."""
import pytest
import torch

import attn_bwd_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def poisoned_lds():
    """Every test starts from LDS full of NaN patterns (see test_dit_backward_gpu.py)."""
    from dgs_amd.dit import DitOps
    DitOps().poison_lds()
    yield


def _ops_and_poison():
    """A DitOps, and its poison_lds to call in front of every attention launch of a case: a fragment read that overtakes its staging
    store then finds NaN patterns, not the previous launch's -- identical -- tile."""
    from dgs_amd.dit import DitOps
    ops = DitOps()
    return ops, ops.poison_lds


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_attention_backward_edge_case(case):
    ops, poison = _ops_and_poison()
    U.check_case(ops, U.case_data(case, False, DEV), before_launch=poison)
    torch.cuda.empty_cache()


def test_attention_backward_edge_case_with_outlier_rows():
    """A q row and the k row L - 1 times 8 (the forward test's outliers): the rounding model alone reaches 0.19 on a 64-row tile and
    0.27 on a row there, so this case is held to the (sample, head) slice bar only -- plus padding, determinism, D, by-products, guards."""
    ops, poison = _ops_and_poison()
    U.check_case(ops, U.case_data(U.OUTLIER_CASE, True, DEV), fine=False, before_launch=poison)
