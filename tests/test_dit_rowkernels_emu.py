"""The DiT row kernels on the CPU emulator build, kernel by kernel against fp64 (rowkernel_util: the harness, the references, the
bars), at the small cases -- and the conditions under which those bars mean something: every reference-only test below applies one
wrong-kernel mutant to the fp64 reference and asserts that the bar is smaller than half of the change it makes (change / bar > 2), on
the inputs the kernel tests use.  The full case list runs on the GPU (test_dit_rowkernels_gpu.py)."""
import pytest
import torch

import rowkernel_util as R
from emu_util import emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


# ---- kernels on the emulator --------------------------------------------------------------------------------------------------------
def test_layernorm(lib):
    R.check_layernorm(lib, "cpu", widths=(256, 1024), shapes=R.LN_SHAPES[:1])


def test_rowlinear(lib):
    R.check_rowlinear(lib, "cpu", Ms=(1, 3, 16), Ns=(14, 37), Ks=(256, 512, 1024))


def test_layernorm_backward(lib):
    """column-sum subsets: dshift alone, dscale + dweight (the first quantity skipped), all three"""
    R.check_layernorm_backward(lib, "cpu", widths=(256, 1024), Bs=(1, 3), rpbs=(5, 24), masks=(1, 6, 7))


def test_rowlinear_backward(lib):
    R.check_rowlinear_backward(lib, "cpu", shapes=[(3, 70, 256), (8, 257, 1024)], per_shape=9)


def test_gate_mul(lib):
    R.check_gate_mul(lib, "cpu", cases=[(3, 64, 64)])


def test_token_scatter_gather(lib):
    R.check_tokens(lib, "cpu", 256)


def test_refusals(lib):
    R.check_refusals(lib, "cpu")


# ---- reference only: what the bars can tell apart -----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", R.LN_WIDTHS)
def test_layernorm_bars_catch_the_mutants(width):
    """One-pass fp32 variance, the neighbouring sample's shift / scale, rows_per_batch off by one: each moves some element by more
    than twice its bar (the f32 output's check), and its nearest-even bf16 fails the bf16 rule at some element, at both shapes and eps."""
    for rows, rpb in R.LN_SHAPES:
        B = R.ceil_div(rows, rpb)
        x, w, mod = R.ln_inputs(rows, width, B, R.LN_SEED + width + rows, "cpu")
        x, w, sh, sc = x.double(), w.double(), mod[:, :width].double(), mod[:, width:2 * width].double()
        for eps in R.LN_EPS:
            ref, bar = R.ref_layernorm(x, w, sh, sc, rpb, eps)
            mutants = {"one-pass fp32 variance": R.one_pass_variance_fp32_layernorm(x, w, sh, sc, rpb, eps),
                       "neighbouring sample's shift": R.ref_layernorm(x, w, sh.roll(1, 0), sc, rpb, eps)[0],
                       "neighbouring sample's scale": R.ref_layernorm(x, w, sh, sc.roll(1, 0), rpb, eps)[0],
                       "rows_per_batch + 1": R.ref_layernorm(x, w, sh, sc, rpb + 1, eps)[0]}
            for name, mut in mutants.items():
                r = R.change_over_bar(mut, ref, bar)
                assert r > 2.0 and R.bf16_rule_catches(mut, ref, bar) > 0, (name, width, rows, eps, r)
            # the statistics alone (no weight, no modulate: the widths' other forms), one-pass variance
            ref, bar = R.ref_layernorm(x, None, None, None, rpb, eps)
            mut = R.one_pass_variance_fp32_layernorm(x, None, None, None, rpb, eps)
            r = R.change_over_bar(mut, ref, bar)
            assert r > 2.0 and R.bf16_rule_catches(mut, ref, bar) > 0, ("one-pass fp32 variance, plain", width, rows, eps, r)


def test_layernorm_bar_is_per_row():
    """The row with mean 1000 has a bar well above its neighbours': one tensor-wide bar would be too loose for them or too tight for it."""
    x, w, mod = R.ln_inputs(21, 1024, 3, 0, "cpu")
    _, bar = R.ref_layernorm(x.double(), None, None, None, 7, 1e-6)
    rowbar = bar.max(-1).values
    others = torch.cat([rowbar[:10], rowbar[11:]])
    assert float(rowbar[10]) > 10 * float(others.max())


LNB_MUTANT_CASES = [(1, 5, 256, 6), (3, 24, 1024, 6), (3, 64, 512, 256), (4, 4224, 256, 256)]   # (B, rows per sample, width, CUs)


@pytest.mark.parametrize("B,rpb,width,ncu", LNB_MUTANT_CASES)
def test_layernorm_backward_bars_catch_the_mutants(B, rpb, width, ncu):
    """A row left out of the column sums (every column of dshift, some column of dscale and dweight), sample 0's scale for every sample
    (dx, dweight), up to the training partition's 4224 rows per sample (66 rows per block, 64 slots; at a quarter of its width)."""
    x, w, mod, dh, dx_in = R.lnb_inputs(B, rpb, width, 0, 300 + width + 10 * rpb + B, "cpu")
    x, w, dh, dx_in = x.double(), w.double(), dh.double(), dx_in.double()
    sc = mod[:, width:2 * width].double()
    rpblk = R.ln_rows_per_block(rpb, B * rpb, ncu)
    if rpb == 4224:
        assert rpblk == 66
    ref = R.ref_ln_backward(x, dh, w, sc.repeat_interleave(rpb, 0), 1e-6, dx_in, B, rpb, rpblk)
    drop = dh.clone()
    drop[B * rpb - 2] = 0.0
    mut = R.ref_ln_backward(x, drop, w, sc.repeat_interleave(rpb, 0), 1e-6, dx_in, B, rpb, rpblk)
    b = B - 1
    change = (mut["dshift"][0][b] - ref["dshift"][0][b]).abs() / ref["dshift"][1][b]
    assert float(change.min()) > 2.0, ("dshift: a dropped row", float(change.min()))
    for name in ("dscale", "dweight"):
        r = R.change_over_bar(mut[name][0], *ref[name])
        assert r > 2.0, (name, "a dropped row", r)
    if B > 1:
        mut = R.ref_ln_backward(x, dh, w, sc[:1].repeat_interleave(B * rpb, 0), 1e-6, dx_in, B, rpb, rpblk)
        for name in ("dx", "dweight"):
            r = R.change_over_bar(mut[name][0], *ref[name])
            assert r > 2.0, (name, "sample 0's scale", r)


def test_column_sum_bar_against_a_dropped_row_of_the_training_partition():
    """Same-signed terms 0.5 + rand: a dropped row of T moves the sum by at least 1 / (3 T) of it.  A sample's sums (T = 4,224, 64 slots:
    depth 9 + 8 + 16 + 2) have a bar of 2.1e-6 of the sum against 7.9e-5; a sum over all T = 16,896 rows (256 slots: depth 9 + 8 + 64 + 2)
    4.9e-6 against 2.0e-5: in both the bar is less than half the change."""
    for T, slots in ((4224, 64), (16896, 256)):
        depth = R.ceil_div(66, 8) + 8 + R.ceil_div(slots, 4) + 2
        assert depth * R.U < 0.5 / (3 * T)


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("K", [256, 512, 1024, 2048])
def test_rowlinear_bar_catches_a_dropped_lane_chunk(M, K):
    """One lane's 8-column chunk of one K step left out of a feature's dot product: every form, N = 14 and 37."""
    for N in (14, 37):
        x, W, bias = R.rowlinear_inputs(M, N, K, "cpu")
        x, W, bias = x.double(), W.double(), bias.double()
        Wm = W.clone()
        lane = 31 if K == 256 else 63
        k0 = (R.ceil_div(K, 512) - 1) * 512 + lane * 8                # the lane's chunk of the last K step
        Wm[N - 1, k0:k0 + 8] = 0.0
        assert not torch.equal(Wm, W)
        for silu_in in (0, 1):
            for silu_out in (0, 1):
                for b in (None, bias):
                    ref, bar = R.ref_rowlinear(x, W, b, silu_in, silu_out)
                    mut, _ = R.ref_rowlinear(x, Wm, b, silu_in, silu_out)
                    assert torch.equal(mut[:, :N - 1], ref[:, :N - 1])
                    r = R.change_over_bar(mut, ref, bar)
                    assert r > 2.0, (M, N, K, silu_in, silu_out, r)


def test_gate_mul_bars_catch_the_mutants():
    """A row left out of dgate and of dbias moves every column by more than twice its bar; the neighbouring sample's gate moves dy."""
    for B, rows, width in ((3, 64, 64), (3, 192, 1024)):
        dx, y, mod = R.gate_inputs(B, rows, width, "cpu")
        dx, y, gate = dx.double(), y.double(), mod[:, 2 * width:3 * width].double()
        ref = R.ref_gate_mul(dx, y, gate, B, rows)
        drop = dx.clone()
        drop[B * rows - 3] = 0.0
        mut = R.ref_gate_mul(drop, y, gate, B, rows)
        change = (mut["dgate"][0][B - 1] - ref["dgate"][0][B - 1]).abs() / ref["dgate"][1][B - 1]
        assert float(change.min()) > 2.0
        rounded = lambda t: t.float().to(torch.bfloat16).double()
        sum_ref, bar = R.ref_gate_dbias(rounded(ref["dy"][0]), B, rows)
        sum_mut, _ = R.ref_gate_dbias(rounded(mut["dy"][0]), B, rows)
        assert float(((sum_mut - sum_ref).abs() / bar).min()) > 2.0
        mut = R.ref_gate_mul(dx, y, gate.roll(1, 0), B, rows)
        assert R.bf16_rule_catches(mut["dy"][0], *ref["dy"]) > 0


def test_bf16_rule_on_an_fp32_layernorm():
    """The bf16 rule applied to torch's own fp32 LayerNorm: no element fails it and few need the midpoint exception
    (less than half the cap: the rule is attainable by a correct fp32 kernel); a value one bf16 step off fails it."""
    for width in R.LN_WIDTHS:
        x, w, mod = R.ln_inputs(21, width, 3, R.LN_SEED + width + 21, "cpu")
        ref, bar = R.ref_layernorm(x.double(), w.double(), None, None, 7, 1e-6)
        got = torch.nn.functional.layer_norm(x, (width,), w, None, 1e-6).to(torch.bfloat16)
        bad, took, _ = R.bf16_verdict(got, ref, bar)
        assert not bool(bad.any()) and float(took.double().mean()) <= R.EXCEPTION_CAP / 2
        off = (got.view(torch.int16) + 1).view(torch.bfloat16)
        bad, _, _ = R.bf16_verdict(off, ref, bar)
        assert float(bad.double().mean()) > 0.9
