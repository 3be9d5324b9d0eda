/* dgs_sampler.h -- C ABI of the diffusion sampler step: the elementwise update that follows the
 * denoiser + rasterizer in every iteration of the sampling loop; and of the training side's counterpart, the inputs of a training
 * step from a clean batch (DgsTrainInputsArgs, below).
 *
 * Replaces, for the configuration the reference ships (create_diffusion: predict_xstart=True, learn_sigma=False;
 * diffusionGS/models/diffusion/__init__.py:15-51), the tensor-op chain of
 *     GaussianDiffusion.p_mean_variance   gaussian_diffusion.py:316-460  (x0 = clamp(model_output, -1, 1); posterior mean)
 *     GaussianDiffusion.q_posterior_mean_variance   :291-313
 *     GaussianDiffusion.p_sample          :479-518                        (x_{t-1} = mean + [t != 0] exp(0.5 log_var) noise)
 * which rebuilds numpy -> tensor coefficient tables four times per step (_extract_into_tensor, :853-866).  Here the tables
 * live on the device, the timestep index is read on the device (no host synchronisation), one launch per step.
 * Plain pointers and sizes only; device pointers; returns DGS_OK or a negative DgsStatus.
 */
#ifndef DGS_SAMPLER_H
#define DGS_SAMPLER_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DgsSamplerStepArgs {
    int32_t B;                 /* samples                                                                             */
    int64_t per_sample;        /* elements per sample of x_t / noise / out ((V-1) * C * H * W)                        */
    int64_t model_stride;      /* elements between samples of model_output (V * C * H * W when it is the render)       */
    int64_t model_offset;      /* first predicted element inside a sample of model_output (C * H * W: view 0 is the
                                  conditioning view, render_imgs[:, 1:] is the prediction; gaussian_diffusion.py:351)   */
    const float* model_output; /* f32: the denoiser's x0 prediction (the rendered views)                              */
    const float* x_t;          /* f32 [B, per_sample]: current noisy views (input_batch["image_noisy"])               */
    const float* noise;        /* f32 [B, per_sample]: N(0, 1) draws (th.randn_like(x), :504); may be NULL iff every t is 0 */
    const int64_t* t;          /* [B] loop indices into the (respaced) tables                                         */
    const float* coef1;        /* [T] posterior_mean_coef1 (multiplies x0)                                            */
    const float* coef2;        /* [T] posterior_mean_coef2 (multiplies x_t)                                           */
    const float* sigma;        /* [T] exp(0.5 * model log-variance)                                                   */
    int32_t T;                 /* table length; t[b] outside [0, T) -> DGS_ERR_INVALID_ARGUMENT is NOT detectable on the
                                  device without a sync: such a sample is left untouched and flagged in *bad_t (if given) */
    int32_t clip_denoised;     /* clamp x0 to [-1, 1] (the reference's default)                                       */
    float* out;                /* f32 [B, per_sample]: x_{t-1}; may alias x_t                                         */
    float* pred_xstart;        /* optional f32 [B, per_sample]: the (clipped) x0                                      */
    int32_t* bad_t;            /* optional device int: set to 1 when some t[b] is out of range                        */
} DgsSamplerStepArgs;

int dgs_sampler_step(const DgsSamplerStepArgs* args, dgs_stream_t stream);

/* The inputs of one TRAINING step from a clean batch, one launch (csrc/sampler.hip).  Replaces
 *     sel_images[:, 1:] = diffusion_training.q_sample(sel_images[:, 1:], timesteps, noise=noise[:, 1:])   diffusion_gs_system.py:87
 *     gt_img_aligned_xyz = ray_o + ray_d * batch['depths_input']                                           diffusion_gs_system.py:88
 *     GaussianDiffusion.q_sample                                                                           gaussian_diffusion.py:268-289
 * on [B, V, 3, H, W] fp32 tensors:
 *     out_image[b, v <  clean_views] = image[b, v]                                 (clean_views = 1: the conditioning view stays clean)
 *     out_image[b, v >= clean_views] = sqrt_acp[t[b]] * image[b, v] + sqrt_1m_acp[t[b]] * noise[b, v]
 *     out_gt_xyz[b, v, c]  = ray_o[b, v, c] + ray_d[b, v, c] * depth[b, v, 0]     (optional, all V views)
 * in the reference's order -- two fp32 products and one fp32 sum, one product and one sum; the file is built without contraction --
 * so both outputs carry the bits of the torch expressions.  The tables are the fp64 schedule rounded to fp32, which is what
 * `_extract_into_tensor(...).float()` (gaussian_diffusion.py:853-866) multiplies with.  t is read on the device: a sample whose t[b]
 * is outside [0, T) keeps its noisy views of out_image unwritten and sets *bad_t (the convention of dgs_sampler_step); its clean views
 * and its xyz target are written all the same.  V == clean_views (V == 1 in training) copies only and never looks at t; clean_views = 0
 * is q_sample on its own.
 * H * W must be a multiple of 4 (16-byte lanes; so must noise_stride and noise_offset).  depth needs ray_o, ray_d and out_gt_xyz;
 * without depth the other three are ignored. */
typedef struct DgsTrainInputsArgs {
    int32_t B, V, H, W;
    int32_t clean_views;       /* leading views that are copied, 0 .. V: 1 in the reference's training step                  */
    const float* image;        /* f32 [B, V, 3, H, W]: the clean views (batch['rgbs_input'])                                 */
    const float* noise;        /* f32: N(0, 1) draws, addressed like DgsSamplerStepArgs.model_output; unused (may be NULL) when V == clean_views */
    int64_t noise_stride;      /* elements between samples of noise: V * 3 * H * W for the reference's full draw
                                  (torch.randn_like(sel_images), :77), (V - 1) * 3 * H * W for a draw of the noisy views only  */
    int64_t noise_offset;      /* first element of the first noisy view's noise inside a sample: 3 * H * W for the full draw
                                  (noise[:, 1:]), 0 otherwise                                                                */
    const int64_t* t;          /* [B] timesteps; unused (may be NULL) when V == clean_views                                  */
    const float* sqrt_acp;     /* [T] sqrt_alphas_cumprod                                                                   */
    const float* sqrt_1m_acp;  /* [T] sqrt_one_minus_alphas_cumprod                                                         */
    int32_t T;
    float* out_image;          /* f32 [B, V, 3, H, W]; may BE image (the reference noises in place): the clean views are then not touched */
    const float* depth;        /* optional f32 [B, V, 1, H, W] (batch['depths_input'])                                       */
    const float* ray_o;        /* f32 [B, V, 3, H, W], with depth                                                            */
    const float* ray_d;        /* f32 [B, V, 3, H, W], with depth                                                            */
    float* out_gt_xyz;         /* f32 [B, V, 3, H, W], with depth                                                            */
    int32_t* bad_t;            /* optional device int: set to 1 when some t[b] is out of range                              */
} DgsTrainInputsArgs;

int dgs_train_inputs(const DgsTrainInputsArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
