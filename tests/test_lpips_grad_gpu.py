"""The LPIPS input gradient on the MI355X (product library): every check of tests/lpips_grad_util.py, all five whole-network cases
included, and one training step with the module as the trainer's perceptual term against the fp32 torch restatement (same weights,
torch autograd) in that place, from the same seed.

Trainer bars.  The step runs three times from the same seed, with three forms in the perceptual slot: the module, the fp32 torch
restatement (F.conv2d in fp32, torch autograd) and the same restatement evaluated in fp64 (the yardstick; the rest of the step is the
same fp32 code on the same bytes, and the test asserts that all three forms saw the same images).
  loss_lpips   the scalar bar of tests/lpips_util.py: |d - d64| <= 8 |d32 - d64| + (512 + H W + 16) 2^-24 d64, H W = 256^2
  gradient     the flat parameter gradient of the step (diffusion term, identical in all runs, plus 0.5 x the perceptual term):
               relative L2 of (module - fp64 form) <= 8 x relative L2 of (fp32 torch form - fp64 form), the fp32 forms' spread measured
               on this very case.  It is not the 1.5e-6 to 2.6e-6 of the small NET_CASES: at 256^2 an image has 17.7 M ReLU inputs, a
               handful of which change sign under fp32 rounding, and each such flip removes or adds a path of the gradient (the
               relative L2 between two fp32 forms is of the order of sqrt(flips / activations), 1e-3 here).  Both values are printed.
"""
import pytest
import torch

import lpips_grad_util as GU
import lpips_util as LU

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("epilogue", [0, 1], ids=["plain", "mask_add"])
@pytest.mark.parametrize("case", GU.CONV_GRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_data_gradient_is_exact_on_gpu(case, epilogue):
    GU.check_conv_grad_exact(DEV, *case, epilogue)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GU.POOL_GRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pool_backward_is_exact_on_gpu(case):
    GU.check_pool_backward_exact(DEV, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GU.TAP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_tap_backward_against_fp64_on_gpu(case):
    GU.check_tap_backward(DEV, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GU.NET_CASES, ids=lambda c: "x".join(map(str, c)))
def test_network_gradient_against_fp64_on_gpu(case):
    GU.check_network_grad(DEV, *case)


@pytest.mark.gpu
@pytest.mark.parametrize("which", GU.PROPERTIES)
def test_gradient_properties_bitwise_on_gpu(which):
    GU.check_property(DEV, which)


@pytest.mark.gpu
def test_surface_on_gpu():
    GU.check_surface(DEV)


@pytest.mark.gpu
def test_train_step_with_the_module_as_the_perceptual_term():
    import train_objective_util as U
    from dgs_amd import sampler
    from dgs_amd.train import DataParallelTrainer
    dev = torch.device(DEV)
    sd = LU.random_state_dict(0)
    module = GU.grad_model(DEV)
    seen = {}

    def with_module(x, y):
        seen["x"], seen["y"] = x.detach().clone(), y.detach().clone()
        assert x.requires_grad and not y.requires_grad
        return module(x, y)

    def with_torch_ops(x, y):
        assert LU.same_bytes(x.detach(), seen["x"]) and LU.same_bytes(y.detach(), seen["y"])
        return LU.restatement_impl(sd, x, y, torch.float32, lambda t: t.to(dev, torch.float32))[0]

    def with_torch_ops_in_fp64(x, y):
        assert LU.same_bytes(x.detach(), seen["x"]) and LU.same_bytes(y.detach(), seen["y"])
        out = LU.restatement_impl(sd, x, y, torch.float64, lambda t: t.to(dev, torch.float64))[0]
        seen["d64"] = float(out.detach().mean())
        return out.float()

    batch = U.clean_batch(1, 2, 2, 16, dev)
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(1, 2, 3, 16, 16, generator=g).to(dev)
    t = torch.tensor([300], dtype=torch.int64, device=dev)
    d = sampler.create_diffusion("1000", device=dev)
    got = []
    for perceptual in (with_module, with_torch_ops, with_torch_ops_in_fp64):
        m = U.small_model(dev, None)
        with DataParallelTrainer(m, torch.optim.SGD(m.parameters(), lr=0.0), bucket_bytes=1 << 20) as tr:
            tr.configure_objective(d, dict(lambda_diffusion=1.0, lambda_lpips=0.5), perceptual=perceptual)
            tr.train_step(batch, noise=noise, timesteps=t)
            assert tr.last_terms["lambda_lpips"] == 0.5
            got.append((float(tr.last_terms["loss_lpips"]), tr.fg.flat.detach().clone()))
    assert tuple(seen["x"].shape) == (2, 3, 256, 256)
    d64 = seen["d64"]
    (a, ga), (b, gb), (_, gc) = got
    bar = LU.FEATURE_FACTOR * abs(b - d64) + (512 + 256 * 256 + 16) * LU.U * d64
    e, e32 = LU.rel_l2(ga, gc), LU.rel_l2(gb, gc)
    print(f"train step: loss_lpips module {a:.8e}, torch ops {b:.8e}, fp64 {d64:.8e}: |module - fp64| / bar = {abs(a - d64) / bar:.4f}")
    print(f"train step: parameter gradient against the fp64 form: module {e:.3e}, fp32 torch ops {e32:.3e}: measured / bar = {e / (8 * e32):.4f}")
    assert a > 0 and abs(a - d64) <= bar
    assert bool(torch.isfinite(ga).all()) and float(ga.norm()) > 0 and e <= LU.FEATURE_FACTOR * e32
