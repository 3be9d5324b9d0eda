/* dgs_loss.h -- C ABI of the image-space loss consumer: the op either side of the rasterizer
 * backward in a training step.
 *
 * Replaces the per-sample L2 / PSNR terms of diffusionGS/utils/losses.py:
 *     per_element_loss = F.mse_loss(rendering, target, reduction='none'); l2_loss = mean over (v, c, h, w)   :281-285
 *     psnr = -10 * log10(l2_loss)                                                                           :303
 *     compute_psnr: clamp both to [0, 1] first                                                               :399-402
 * and the autograd backward of the lambda_mse term (d/d rendering = 2 (rendering - target) * grad_scale / n).
 * and the SSIM term (`SsimLoss`, :216-234; evaluated over all b * v views on every step, :317-321): DgsSsimArgs below.
 * The LPIPS network, forward and input gradient, is include/dgs_lpips.h (csrc/lpips.hip; the metric of MetricComputer and the
 * LPIPS TERM of the loss): its input path is DgsResizeArgs here, and the trainer's slot takes it or any differentiable network
 * (DataParallelTrainer.configure_objective(perceptual=...)).  One pass over the images, per-sample
 * sums reduced in a fixed order (deterministic), no host synchronisation.  Device pointers; returns DGS_OK or a negative DgsStatus.
 */
#ifndef DGS_LOSS_H
#define DGS_LOSS_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define DGS_LOSS_CHUNKS 64 /* partial sums per sample */

typedef struct DgsMseArgs {
    int32_t B;                 /* samples                                                                  */
    int64_t n;                 /* elements per sample (v * 3 * h * w), a multiple of 4                     */
    const float* rendering;    /* f32 [B, n]                                                               */
    const float* target;       /* f32 [B, n]                                                               */
    int32_t clamp01;           /* clamp both to [0, 1] before the difference (compute_psnr, :399-400)       */
    float* l2;                 /* out f32 [B]: mean squared error per sample                               */
    float* psnr;               /* optional out f32 [B]: -10 log10(l2)                                      */
    float* grad;               /* optional out f32 [B, n]: grad_scale * 2 (rendering - target) / n          */
    float grad_scale;          /* e.g. lambda_mse / B for the batch-mean loss                              */
    float* partial;            /* workspace f32 [B, DGS_LOSS_CHUNKS]                                        */
} DgsMseArgs;

int dgs_mse_psnr(const DgsMseArgs* args, dgs_stream_t stream);

/* The input path of the LPIPS term (losses.py:304-309): `F.interpolate(x, size=[256, 256], mode='bilinear') * 2.0 - 1.0`
 * for renderings and targets -- evaluated every step, also when lambda_lpips is 0.  One launch: bilinear resize
 * (align_corners = False, PyTorch's source-index rule) fused with the affine map; the backward accumulates
 * d src = mul * W^T d dst (dsrc is zero-filled by the call).  The network behind it: include/dgs_lpips.h. */
typedef struct DgsResizeArgs {
    int32_t planes;            /* n * c image planes                                                       */
    int32_t in_h, in_w, out_h, out_w;
    const float* src;          /* f32 [planes, in_h, in_w]       (forward)                                 */
    float* dst;                /* f32 [planes, out_h, out_w]     (forward)                                 */
    float mul, add;            /* dst = resize(src) * mul + add                                            */
    const float* ddst;         /* f32 [planes, out_h, out_w]     (backward)                                */
    float* dsrc;               /* f32 [planes, in_h, in_w]       (backward, written)                       */
} DgsResizeArgs;

int dgs_resize_bilinear(const DgsResizeArgs* args, dgs_stream_t stream);
int dgs_resize_bilinear_backward(const DgsResizeArgs* args, dgs_stream_t stream);

/* The two loss terms on the denoiser's pixel-aligned points `img_aligned_xyz` (losses.py:288-292, 325-364; `lambda_pointsdist: 1.0`
 * is the only active term of the first training steps of configs/diffusionGS_rel.yaml), forward values and the gradient with
 * respect to `aligned` in two passes over the tensors, every sum reduced in a fixed order:
 *   points-distribution loss, per sample b:
 *       dist = |aligned - ray_o|_2 per pixel; per (b, view): mean and UNBIASED std of dist over the view's pixels (detached; summed
 *       on dist minus the view's first distance, so that nearly constant distances -- those first steps -- do not cancel in fp32; a
 *       view of one pixel has std 0);
 *       target = (dist - mean) / (std + 1e-8) * 0.5 + |ray_o|_2;   pointsdist[b] = mean over (v, h, w) of (dist - target)^2
 *   xyz loss, one scalar for the batch (optional: gt and masks given):
 *       xyz = sum((aligned * m - gt * m)^2) / sum(m),  m = masks [B, V, 1, H, W] broadcast over the three coordinates
 *   grad = w_pointsdist[b] * d pointsdist[b] / d aligned + w_xyz * d xyz / d aligned      (optional)
 * Called by the trainer's objective (dgs_amd.train.DataParallelTrainer.train_step through losses.points_losses /
 * points_losses_part), whose gradient reaches dgs_dit_backward as d / d img_aligned_xyz.                                         */
typedef struct DgsPointsLossArgs {
    int32_t B, V, H, W;
    const float* aligned;      /* f32 [B, V, 3, H, W]                                                       */
    const float* ray_o;        /* f32 [B, V, 3, H, W]                                                       */
    const float* gt;           /* optional f32 [B, V, 3, H, W]                                              */
    const float* masks;        /* optional f32 [B, V, 1, H, W] (required with gt)                            */
    float* pointsdist;         /* out f32 [B]                                                               */
    float* xyz;                /* out f32 [1] (written when gt is given)                                    */
    const float* w_pointsdist; /* optional f32 [B]: upstream gradient of pointsdist[b] (NULL: 0)             */
    float w_xyz;               /* upstream gradient of xyz                                                  */
    float* grad;               /* optional out f32 [B, V, 3, H, W]                                          */
    float* workspace;          /* f32 [dgs_points_loss_workspace_floats(B, V)]                               */
    /* appended (a zero-initialised tail is the call as it was): what a trainer needs to evaluate a batch in micro-batches without
       reading a device value back to the host */
    const float* xyz_denominator; /* optional device f32 [1]: stands in for sum(m) in xyz and its gradient (the mask sum of the WHOLE
                                     batch when this call sees a part of it: the parts' xyz then add up to the batch's)  */
    const float* w_xyz_dev;    /* optional device f32 [1]: multiplies w_xyz (an upstream gradient that lives on the device) */
} DgsPointsLossArgs;

int64_t dgs_points_loss_workspace_floats(int32_t B, int32_t V);
int dgs_points_loss(const DgsPointsLossArgs* args, dgs_stream_t stream);

/* SSIM of the reference's SsimLoss (losses.py:216-234: pytorch_msssim.SSIM(win_size=11, win_sigma=1.5, data_range=1.0,
 * size_average=False, channel=3)), forward and backward with respect to x, fused with the MSE term (csrc/ssim.hip):
 *     w[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0 .. 10, normalised to sum 1 (fp32);  G = separable VALID filter with w along H, then W
 *     mu1 = G(x), mu2 = G(y), s1 = G(x x) - mu1^2, s2 = G(y y) - mu2^2, s12 = G(x y) - mu1 mu2,  C1 = (0.01 R)^2, C2 = (0.03 R)^2
 *     m = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * (2 s12 + C2) / (s1 + s2 + C2);   ssim[n] = mean of m over C (H - 10) (W - 10)
 * dgs_ssim: one tiled launch (no moment map goes to memory; with `saved` the three partial-derivative maps of the backward are
 * written) + one finishing launch that adds the tile sums in index order.  With `l2` it also emits dgs_mse_psnr's per-sample
 * l2 / psnr of (x, y) (clamp01 = 0), samples being groups of V = N / B consecutive images.
 * dgs_ssim_backward: one launch, a gather over `saved` (no atomics):
 *     dx = g[n] * d ssim[n] / d x  +  mse_scale[b] * 2 (x - y) / (V C H W)
 * Same inputs, same bits.  H < 11 or W < 11 (or N * C > 65535 planes in one call): DGS_ERR_INVALID_ARGUMENT. */
typedef struct DgsSsimArgs {
    int32_t N, C, H, W;        /* images, channels, plane size                                              */
    int32_t B;                 /* samples: N = B * V (a divisor of N; only the MSE outputs / mse_scale use it) */
    const float* x;            /* f32 [N, C, H, W]: the renderings (differentiated)                          */
    const float* y;            /* f32 [N, C, H, W]: the targets                                              */
    float data_range;          /* R: 1.0 in the reference                                                    */
    float* ssim;               /* forward out f32 [N]                                                        */
    float* l2;                 /* forward optional out f32 [B]: mean squared error per sample                */
    float* psnr;               /* forward optional out f32 [B]: -10 log10(l2) (needs l2)                      */
    float* saved;              /* f32 [dgs_ssim_saved_floats(N, C, H, W)], layout private to the library: written by the forward
                                  when given, REQUIRED by the backward                                      */
    float* workspace;          /* forward: f32 [dgs_ssim_workspace_floats(N, C, H, W)]                        */
    const float* g;            /* backward: f32 [N], d L / d ssim[n]                                          */
    const float* mse_scale;    /* backward optional f32 [B]: d L / d l2[b]                                    */
    float* dx;                 /* backward out f32 [N, C, H, W]                                               */
} DgsSsimArgs;

int64_t dgs_ssim_workspace_floats(int32_t N, int32_t C, int32_t H, int32_t W);
int64_t dgs_ssim_saved_floats(int32_t N, int32_t C, int32_t H, int32_t W);
int dgs_ssim(const DgsSsimArgs* args, dgs_stream_t stream);
int dgs_ssim_backward(const DgsSsimArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
