"""The DiT row kernels on MI355X, kernel by kernel against fp64 (rowkernel_util: harness, references, bars and the full case lists).
The GPU runs code the emulator never runs: wave_sum as a chain of DPP adds read back from lane 63, pack_bf2 / f2bf_fast as
v_cvt_pk_bf16_f32, the LayerNorm backward's partition by the real CU count -- and several instantiations no other GPU test reaches:
LayerNorm widths 256, 512, 768 and 2048 in their eight weight / modulate / output forms, rowlinear_kernel<4>, <8>, <16> with M < MR,
layernorm_backward_kernel<1> and <2>, f32 dh, every subset of the three column sums.  LDS is poisoned in front of every launch.
Measured error / bar per case and output: profiles/dit_rowkernels_parity.txt (tools/dit_rowkernel_error.py)."""
import pytest
import torch

import rowkernel_util as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def poisoned_lds():
    """Every test starts from LDS full of NaN patterns (see test_dit_gpu.py)."""
    from dgs_amd.dit import DitOps
    DitOps().poison_lds()
    yield


def _lib_and_poison():
    from dgs_amd.dit import DitOps
    ops = DitOps()
    return ops.lib, ops.poison_lds


@pytest.mark.parametrize("width", R.LN_WIDTHS)
def test_layernorm(width):
    lib, poison = _lib_and_poison()
    R.check_layernorm(lib, DEV, widths=(width,), before=poison)


@pytest.mark.parametrize("N", R.RL_NS)
def test_rowlinear(N):
    lib, poison = _lib_and_poison()
    R.check_rowlinear(lib, DEV, Ns=(N,), before=poison)


@pytest.mark.parametrize("width", R.LNB_WIDTHS)
def test_layernorm_backward(width):
    lib, poison = _lib_and_poison()
    R.check_layernorm_backward(lib, DEV, widths=(width,), before=poison)


def test_layernorm_backward_training_partition():
    lib, poison = _lib_and_poison()
    R.check_layernorm_backward_training_partition(lib, DEV, before=poison)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("N", R.RLB_NS)
def test_rowlinear_backward(N):
    lib, poison = _lib_and_poison()
    R.check_rowlinear_backward(lib, DEV, shapes=[(M, N, K) for K in R.RLB_KS for M in R.RLB_MS], before=poison)


def test_gate_mul():
    lib, poison = _lib_and_poison()
    R.check_gate_mul(lib, DEV, before=poison)


def test_token_scatter_gather():
    lib, poison = _lib_and_poison()
    R.check_tokens(lib, DEV, 1024, before=poison)


def test_refusals():
    lib, poison = _lib_and_poison()
    R.check_refusals(lib, DEV, before=poison)
