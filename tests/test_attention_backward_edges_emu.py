"""Attention backward at sequence-length and batch edges on the CPU emulator build (tests/hipemu): the checks of
test_attention_backward_edges_gpu.py -- see there -- through DitOps(lib=emu_lib()) for the cases with L <= 1026, and one test that needs
no kernel: the yardstick those checks use must itself sit well inside the project's bar."""
import pytest

import attn_bwd_util as U
from dgs_amd.dit import DitOps
from emu_util import emu_lib

EMU_CASES = [c for c in U.CASES if c[0] <= U.EMU_MAX_L]


@pytest.fixture(scope="module")
def ops():
    return DitOps(lib=emu_lib())


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_rounding_model_leaves_room_under_the_tensor_bar(case):
    """The accuracy bars are 3 x the rounding model's own error (fp64 with the kernel's five bf16 roundings against exact fp64
    autograd).  They are attainable by a correct kernel, and mean something next to the project's tensor-wide 1.5e-2, only while the
    model itself stays below half of that bar, tensor by tensor."""
    data = U.case_data(case)
    W = data["inp"]["W"]
    for i, name in enumerate(("dq", "dk", "dv")):
        e = U.rel_l2(data["dmod"][:, :, i * W:(i + 1) * W], data["dref"][:, :, i * W:(i + 1) * W])
        print(f"{U.case_id(case)} {name} rounding model rel_l2 {e:.3e}")
        assert e < 0.5 * U.TENSOR_REL_L2, (name, e)
    print({k: f"{v:.3e}" for k, v in U.worst(data["model_err"]).items()})


def test_rounding_model_leaves_room_under_the_slice_bar_with_outlier_rows():
    """The outlier case is held to 1.5e-2 per (tensor, sample, head) slice: its draw (attn_bwd_util.OUTLIER_SEED) is one at which the
    rounding model's worst slice error is below half of that."""
    w = U.worst(U.case_data(U.OUTLIER_CASE, True)["model_err"])
    print({k: f"{v:.3e}" for k, v in w.items()})
    assert w["slice"] < 0.5 * U.TENSOR_REL_L2, w


@pytest.mark.parametrize("case", EMU_CASES, ids=U.case_id)
def test_attention_backward_edge_case(ops, case):
    U.check_case(ops, U.case_data(case))


def test_attention_backward_edge_case_with_outlier_rows(ops):
    """A q row and the k row L - 1 times 8 (the forward test's outliers): the rounding model alone reaches 0.19 on a 64-row tile and
    0.27 on a row there, so this case is held to the (sample, head) slice bar only -- plus padding, determinism, D, by-products, guards."""
    U.check_case(ops, U.case_data(U.OUTLIER_CASE, True), fine=False)
