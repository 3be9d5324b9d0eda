"""Loss, clip, AdamW and sampler kernels on MI355X at the sizes where their index arithmetic changes (tests/step_kernels_util.py holds the
cases, the references and the checks; tests/test_step_kernels_emu.py runs the same on the CPU emulator build).  Every C-level launch
writes between guard bands of 7.0, which must be untouched afterwards.  Per kernel:

  points loss  the seven (base, spread, size) rows from spread 0.5 down to 0.001 of the depth (std of the distances 1.4e-1 .. 2.8e-4):
               loss and gradient, separately, within max(2e-4 of tests/test_losses.py, 4 x the error of the reference's own torch
               expression in fp32 on the CPU) against fp64 of the same inputs.  4: sums of distances shifted by the plane's first one sit
               at 0.3 - 1.6 x that error, 2.5 x is left for another summation order and FMA contraction; the raw sums of d and d^2 this
               kernel had were 80 - 600 x off at the narrow rows (loss 9.5e-2, gradient 1.3e-1 at spread 0.001).  Shape edges (one pixel,
               25 pixels in 64 chunks, 31 x 37, B = V = 1, B = 3 with three weights) with and without gt at 2e-4 / 1e-5; the guarded direct
               call gives the wrapper's bits
  mse / psnr   target 0 and rendering[b] = 2^b: l2[b] == 4^b and gradient == fl(fl(2 grad_scale) / n) 2^b to the bit; n = 12 .. 49152
               against fp64 at 2e-6 (l2), 1e-5 (psnr, gradient); clamp01 with values outside [0, 1]; n = 27 refused, nothing written
  resize       1 x 1, 2 x 3, 257 x 255, 1024 x 768 -> 256 x 256, 245 outputs in all, 32 x 48: within 2e-6 of F.interpolate in fp32 and in
               fp64 (every ratio is dyadic, so the source coordinates are exact), gradient at rtol 1e-4 + 1e-5 max
  sum of sq.   n = 1 .. 2 * 65536 + 1030: all ones and one hot exactly; random data within 265 * 2^-24 of fp64 per partial and in total
               (256 sequential additions per lane, 6 shuffle steps, 3 additions, non-negative terms); the full-chunk and the tail form give
               the same bits; GradNorm out of order and re-added
  adamw        13 tensors (scalar tails, a tile's end, one / 2 x 3 / 3 x 1 transposed blocks), steps 1, 2, 3 and 10000, decay 0 and 0.05,
               clip off (NaN in the unused word) / clipping / not clipping: p, m, v per tensor within max(4 x the error of
               torch.optim.AdamW(foreach=False) in fp32 on the CPU, 2^-23 max|ref|) of fp64 -- both sides are a handful of fp32 roundings
               in another order; a wrong bias correction, decay or tensor is orders of magnitude off -- and within the project's 2e-6
               max|ref|; copies == p.to(bf16) / p / copy.t() bit for bit; dgs_adamw_ema_step gives the same p, m, v bits and the
               reference's shadow; NaN, +inf, -inf in the sum of squares with the clip on leave everything as it is
  sampler      4 (1024 * 256 + 257) elements per sample (a partial second trip of the grid-stride loop), t = [0, T - 1, 7], model offset
               of one view: bit-equal to c1 * x0 + c2 * x, then + sigma * z in fp32 torch (the file is built without contraction), within
               2e-6 of the numpy oracle; in place; no noise at t = 0; t = -1 and t = T flagged and left alone; refusals
Measured: profiles/step_kernels_parity.txt (tools/step_kernels_error.py)."""
import pytest

import step_kernels_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CHECKS = [U.check_points_accuracy, U.check_points_edges, U.check_mse, U.check_resize, U.check_sumsq, U.check_adamw, U.check_sampler_step,
          U.check_sampler_entry]


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_step_kernel_on_gpu(check):
    import torch
    check(None, DEV)
    torch.cuda.synchronize()
