// sampler.hip -- one fused elementwise kernel for the diffusion sampler step and one for the inputs of a training step (q_sample, the xyz
// target; further down) (include/dgs_sampler.h).
// HBM-bound by construction: 3 streams in (model output, x_t, noise), 1-2 out, 16 bytes per lane, no tables on the host.
// Arithmetic order is the reference's (gaussian_diffusion.py:301-304, 504-512): c1 * x0 + c2 * x_t, then + sigma * noise, in
// fp32 without contraction (this file is built with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "dgs_device.h"
#include "dgs_sampler.h"

namespace dgs {

__global__ __launch_bounds__(256) void sampler_step_kernel(DgsSamplerStepArgs a) {
    const int b = blockIdx.y;
    const long long t = a.t[b];
    if (t < 0 || t >= a.T) {
        if (a.bad_t && threadIdx.x == 0 && blockIdx.x == 0) *a.bad_t = 1;
        return;
    }
    const float c1 = a.coef1[t], c2 = a.coef2[t], sg = t != 0 ? a.sigma[t] : 0.0f;
    const float* mo = a.model_output + (size_t)b * a.model_stride + a.model_offset;
    const size_t base = (size_t)b * a.per_sample;
    const long long n4 = a.per_sample / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 m = reinterpret_cast<const float4*>(mo)[i];
        const float4 x = reinterpret_cast<const float4*>(a.x_t + base)[i];
        float4 x0 = m;
        if (a.clip_denoised) {
            x0.x = fminf(fmaxf(m.x, -1.0f), 1.0f); x0.y = fminf(fmaxf(m.y, -1.0f), 1.0f);
            x0.z = fminf(fmaxf(m.z, -1.0f), 1.0f); x0.w = fminf(fmaxf(m.w, -1.0f), 1.0f);
        }
        float4 o = make_float4(c1 * x0.x + c2 * x.x, c1 * x0.y + c2 * x.y, c1 * x0.z + c2 * x.z, c1 * x0.w + c2 * x.w);
        if (t != 0 && a.noise) {
            const float4 z = reinterpret_cast<const float4*>(a.noise + base)[i];
            o.x = o.x + sg * z.x; o.y = o.y + sg * z.y; o.z = o.z + sg * z.z; o.w = o.w + sg * z.w;
        }
        reinterpret_cast<float4*>(a.out + base)[i] = o;
        if (a.pred_xstart) reinterpret_cast<float4*>(a.pred_xstart + base)[i] = x0;
    }
}

// The inputs of a training step (DgsTrainInputsArgs): q_sample of the noisy views, the copy of the clean one and the xyz target, one launch.
// 5 streams in (image, noise, depth, ray_o, ray_d), 2 out, 16 bytes per lane.  blockIdx.y = (b, v), blockIdx.z = the colour / coordinate
// plane, so that a lane's depth index is its own index (depth has one plane per view) and no lane divides.
#define DGS_TRAIN_INPUTS_GRID_X 256   // workgroups per plane before the loop strides: x B V 3 planes this is past the ~2048 a streaming kernel wants

__global__ __launch_bounds__(256) void train_inputs_kernel(DgsTrainInputsArgs a) {
    const int bv = blockIdx.y, c = blockIdx.z;
    const int b = bv / a.V, v = bv - b * a.V;
    const long long hw = (long long)a.H * a.W, n4 = hw / 4;
    const size_t plane = ((size_t)bv * 3 + c) * hw;
    const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    if (a.depth) {
        const float4* dp = reinterpret_cast<const float4*>(a.depth + (size_t)bv * hw);
        for (long long i = first; i < n4; i += stride) {
            const float4 d = dp[i];
            const float4 o = reinterpret_cast<const float4*>(a.ray_o + plane)[i];
            const float4 r = reinterpret_cast<const float4*>(a.ray_d + plane)[i];
            reinterpret_cast<float4*>(a.out_gt_xyz + plane)[i] = make_float4(o.x + r.x * d.x, o.y + r.y * d.y, o.z + r.z * d.z, o.w + r.w * d.w);
        }
    }
    if (v < a.clean_views) {
        if (a.out_image != a.image)
            for (long long i = first; i < n4; i += stride)
                reinterpret_cast<float4*>(a.out_image + plane)[i] = reinterpret_cast<const float4*>(a.image + plane)[i];
        return;
    }
    const long long t = a.t[b];
    if (t < 0 || t >= a.T) {
        if (a.bad_t && threadIdx.x == 0 && blockIdx.x == 0) *a.bad_t = 1;
        return;
    }
    const float ca = a.sqrt_acp[t], cs = a.sqrt_1m_acp[t];
    const float* z = a.noise + (size_t)b * a.noise_stride + a.noise_offset + ((size_t)(v - a.clean_views) * 3 + c) * hw;
    for (long long i = first; i < n4; i += stride) {
        const float4 x = reinterpret_cast<const float4*>(a.image + plane)[i];      // read before the store: out_image may be image
        const float4 n = reinterpret_cast<const float4*>(z)[i];
        reinterpret_cast<float4*>(a.out_image + plane)[i] = make_float4(ca * x.x + cs * n.x, ca * x.y + cs * n.y, ca * x.z + cs * n.z, ca * x.w + cs * n.w);
    }
}

}  // namespace dgs

extern "C" int dgs_train_inputs(const DgsTrainInputsArgs* a, dgs_stream_t stream) {
    if (!a || a->B <= 0 || a->V <= 0 || a->H <= 0 || a->W <= 0 || a->T <= 0 || ((long long)a->H * a->W) % 4 || !a->image || !a->out_image ||
        !a->sqrt_acp || !a->sqrt_1m_acp)
        return DGS_ERR_INVALID_ARGUMENT;
    if (a->clean_views < 0 || a->clean_views > a->V) return DGS_ERR_INVALID_ARGUMENT;
    if (a->V > a->clean_views && (!a->noise || !a->t || a->noise_stride % 4 || a->noise_offset % 4 || a->noise_offset < 0 ||
                     a->noise_stride < a->noise_offset + (long long)(a->V - a->clean_views) * 3 * a->H * a->W))
        return DGS_ERR_INVALID_ARGUMENT;
    if (a->depth && (!a->ray_o || !a->ray_d || !a->out_gt_xyz)) return DGS_ERR_INVALID_ARGUMENT;
    if ((long long)a->B * a->V > 65535) return DGS_ERR_INVALID_ARGUMENT;       // blockIdx.y
    const long long n4 = (long long)a->H * a->W / 4;
    const int gx = (int)((n4 + 255) / 256 < DGS_TRAIN_INPUTS_GRID_X ? (n4 + 255) / 256 : DGS_TRAIN_INPUTS_GRID_X);
    hipLaunchKernelGGL(dgs::train_inputs_kernel, dim3(gx, a->B * a->V, 3), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_sampler_step(const DgsSamplerStepArgs* a, dgs_stream_t stream) {
    if (!a || a->B <= 0 || a->per_sample <= 0 || a->per_sample % 4 || a->model_offset % 4 || a->model_stride % 4 || a->T <= 0 ||
        !a->model_output || !a->x_t || !a->t || !a->coef1 || !a->coef2 || !a->sigma || !a->out)
        return DGS_ERR_INVALID_ARGUMENT;
    const long long n4 = a->per_sample / 4;
    const int gx = (int)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
    hipLaunchKernelGGL(dgs::sampler_step_kernel, dim3(gx, a->B), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
