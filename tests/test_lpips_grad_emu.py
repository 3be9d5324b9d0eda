"""The LPIPS input gradient (csrc/lpips.hip, include/dgs_lpips.h 'The input gradient', dgs_amd.lpips) on the CPU-emulated build of the
kernels: the checks of tests/lpips_grad_util.py, which states the bars.  tests/test_lpips_grad_gpu.py runs the same checks on the GPU.

Trimmed here, because the emulator switches fibers at every MFMA: of the whole-network cases only (2, 16, 16) runs here, the other
four on the GPU; the properties are trimmed as check_property(thorough=False) says.  The trainer's step needs 256^2 images and runs on the GPU only."""
import pytest

import lpips_grad_util as GU

DEV = "cpu"


@pytest.mark.parametrize("epilogue", [0, 1], ids=["plain", "mask_add"])
@pytest.mark.parametrize("case", GU.CONV_GRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_data_gradient_is_exact(case, epilogue):
    GU.check_conv_grad_exact(DEV, *case, epilogue)


@pytest.mark.parametrize("case", GU.POOL_GRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_backward_is_exact(case):
    GU.check_pool_backward_exact(DEV, *case)


@pytest.mark.parametrize("case", GU.TAP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tap_backward_against_fp64(case):
    GU.check_tap_backward(DEV, *case)


def test_network_gradient_against_fp64():
    GU.check_network_grad(DEV, 2, 16, 16)


@pytest.mark.parametrize("which", GU.PROPERTIES)
def test_gradient_properties_bitwise(which):
    GU.check_property(DEV, which, thorough=False)


def test_surface():
    GU.check_surface(DEV)


def test_workspace_is_bounded_in_n():
    GU.check_workspace(GU.lib_of(DEV))


def test_new_structs_match_c_layout():
    import ctypes
    import os
    import subprocess
    import tempfile

    from dgs_amd import _native
    structs = ["DgsConv3x3BackwardDataArgs", "DgsMaxPool2x2BackwardArgs", "DgsLpipsTapBackwardArgs", "DgsLpipsGradArgs"]
    fields = [("DgsConv3x3BackwardDataArgs", "dx"), ("DgsMaxPool2x2BackwardArgs", "dx"), ("DgsLpipsTapBackwardArgs", "g1"),
              ("DgsLpipsGradArgs", "workspace_bytes"), ("DgsLpipsGradArgs", "conv_wt"), ("DgsLpipsGradArgs", "grad0")]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "dgs_lpips.h"\nint main(){' + "".join(f'printf("%zu\\n", sizeof({s}));' for s in structs) + "".join(
        f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(GU.LU.ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [ctypes.sizeof(getattr(_native, s)) for s in structs] + [getattr(getattr(_native, s), f).offset for s, f in fields]
    assert got == want, (got, want)
