"""The training objective from a clean batch on the GPU (gfx950 build): the cases of tests/test_train_objective_emu.py that run on the
device -- dgs_train_inputs bit for bit between guard bands, train_step against step() bit for bit, one step with every device term.
The comparison with the reference's Python stays on the emulator.  Model: the one of tests/test_ref_callers.py's GPU system case
(width 1024, 4 blocks, 64^2)."""
import pytest
import torch

import train_objective_util as U

GPU_MODEL = dict(width=1024, layers=4, res=64)


def _dev():
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_train_inputs_bits_gpu(shape):
    U.check_train_inputs_shape(None, _dev(), shape)


@pytest.mark.gpu
def test_train_inputs_refusals_gpu():
    U.check_train_inputs_entry(None, _dev())


@pytest.mark.gpu
@pytest.mark.parametrize("lambda_ssim", [None, 0.2], ids=["mse", "mse_ssim"])
def test_train_step_equals_step_bit_for_bit_gpu(lambda_ssim):
    U.check_equivalence_with_step(None, _dev(), lambda_ssim, **GPU_MODEL)


@pytest.mark.gpu
def test_all_terms_gpu():
    U.check_all_terms(None, _dev(), **GPU_MODEL)
