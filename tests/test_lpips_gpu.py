"""The LPIPS-VGG forward on the MI355X (product library): every check of tests/lpips_util.py, all five whole-network cases included,
and the metric path of tests/test_metrics.py on the device.

Not asserted: that the GPU's bytes equal the emulator's.  The suite asserts that for no strict-fp file; here the convolution and the
pool are pinned bit for bit by exact integer data on both, everything else by the same fp64 bars on both."""
import pytest
import torch

import lpips_util as LU
import test_metrics as TM

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", LU.CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_convolution_is_exact_on_gpu(case, relu):
    LU.check_conv_exact(DEV, *case, relu)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LU.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_is_exact_on_gpu(case):
    LU.check_pool_exact(DEV, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LU.TAP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tap_kernel_against_fp64_on_gpu(case):
    LU.check_tap(DEV, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LU.NET_CASES, ids=lambda c: "x".join(map(str, c)))
def test_network_against_fp64_on_gpu(case):
    LU.check_network(DEV, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("which", LU.PROPERTIES)
def test_properties_bitwise_on_gpu(which):
    LU.check_property(DEV, which)


@pytest.mark.gpu
def test_module_moves_to_the_device_and_refuses_a_gradient():
    m = LU.model(DEV)
    assert all(p.is_cuda for p in m.parameters())
    x = torch.zeros(1, 3, 16, 16, device=DEV)
    with pytest.raises(NotImplementedError, match="input gradient"):
        m(x.clone().requires_grad_(True), x)
    with pytest.raises(ValueError, match="16 x 16"):
        m(x[..., :15], x[..., :15])
    assert bool((m(x, x) == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("size", TM.SSIM_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_compute_ssim_on_gpu(size):
    TM.check_ssim(DEV, *size)


@pytest.mark.gpu
def test_compute_psnr_on_gpu():
    TM.check_psnr(DEV)


@pytest.mark.gpu
def test_metric_computer_and_compute_metrics_on_gpu(tmp_path):
    TM.check_forward_and_files(DEV, str(tmp_path))
