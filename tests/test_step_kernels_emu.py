"""Loss, clip, AdamW and sampler kernels at their edges on the CPU emulator build (tests/step_kernels_util.py; the same checks run on
MI355X in tests/test_step_kernels_gpu.py, where the bars are summarised)."""
import pytest

import step_kernels_util as U
from emu_util import emu_lib

CHECKS = [U.check_points_accuracy, U.check_points_edges, U.check_mse, U.check_resize, U.check_sumsq, U.check_adamw, U.check_sampler_step,
          U.check_sampler_entry]


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_step_kernel_on_the_emulator(check):
    check(emu_lib(), "cpu")
