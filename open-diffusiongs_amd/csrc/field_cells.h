// field_cells.h -- the binning of Gaussians into cells of pitch 2 / nb over [-1, 1]^3 and their 48-byte records, shared by field.hip (the
// density on a voxel grid) and mesh_attr.hip (the same records evaluated at mesh vertices).  Moved here from field.hip unchanged: the
// workspace layout, the cell function, the key / scan / scatter / prepare kernels and the compensated exponential.  The kernels are
// `static`: every file that includes this header has its own copy, and the copies do not meet at link time.
//   field_key_kernel      thread = row of a.xyz: the cell of its coordinates, counted per cell
//   field_scan_kernel     one workgroup: exclusive scan of the nb^3 counts -> cell offsets; the counts become the scatter's cursors
//   field_scatter_kernel  thread = row: its index into its cell's segment, at whatever slot the atomic hands out
//   field_prepare_kernel  thread = Gaussian: its rank = the number of smaller indices in its cell's segment (so the order inside a cell
//                         is the index order, whatever the atomics did), then its record at offset + rank: centre, sigmoid(opacity)
//                         and the six coefficients of -1/2 Sigma^-1, Sigma^-1 = R diag(1 / s^2) R^T, evaluated in fp64 and rounded once
// key, scan and scatter read only a.N, a.nb, a.xyz and the four arrays of the FieldWs, so they bin any [N, 3] array of coordinates
// (mesh_attr.hip bins its query points with them through a second FieldWs whose pointers name the points' arrays).
#ifndef DGS_FIELD_CELLS_H
#define DGS_FIELD_CELLS_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "dgs_device.h"
#include "dgs_field.h"

namespace dgs {

constexpr int FIELD_WG = 256;
constexpr int FIELD_MAX_NB = 256;

struct FieldWs {
    uint32_t *count, *offsets, *keys, *index;
    float4* rec;
    int64_t bytes;
    __host__ FieldWs(void* base, int64_t N, int64_t nb) {
        const int64_t cells = nb * nb * nb;
        auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
        char* p = static_cast<char*>(base);
        int64_t at = 0;
        count = reinterpret_cast<uint32_t*>(p + at);   at += up(4 * cells);
        offsets = reinterpret_cast<uint32_t*>(p + at); at += up(4 * (cells + 1));
        keys = reinterpret_cast<uint32_t*>(p + at);    at += up(4 * N);
        index = reinterpret_cast<uint32_t*>(p + at);   at += up(4 * N);
        rec = reinterpret_cast<float4*>(p + at);       at += 48 * N;
        bytes = at;
    }
};

// Cell of a coordinate on the grid of pitch 2 / nb over [-1, 1], clamped; every step is monotone in x, so lo < x < hi implies
// field_cell(lo) <= field_cell(x) <= field_cell(hi).  A NaN lands in cell 0 (and is a member of nothing).
__device__ __forceinline__ int field_cell(float x, int nb) {
    const float t = floorf((x + 1.0f) * (0.5f * (float)nb));
    if (!(t >= 0.f)) return 0;
    if (t > (float)(nb - 1)) return nb - 1;
    return (int)t;
}

static __global__ __launch_bounds__(FIELD_WG) void field_key_kernel(DgsFieldArgs a, FieldWs ws) {
    const int i = blockIdx.x * FIELD_WG + threadIdx.x;
    if (i >= a.N) return;
    const int cx = field_cell(a.xyz[3 * (size_t)i], a.nb), cy = field_cell(a.xyz[3 * (size_t)i + 1], a.nb), cz = field_cell(a.xyz[3 * (size_t)i + 2], a.nb);
    const uint32_t key = ((uint32_t)cx * a.nb + cy) * a.nb + cz;
    ws.keys[i] = key;
    atomicAdd(&ws.count[key], 1u);                       // a count: the same whatever the arrival order
}

static __global__ __launch_bounds__(1024) void field_scan_kernel(FieldWs ws, int64_t cells) {
    __shared__ uint32_t scratch[1024 / DGS_WAVE + 1];
    const int64_t per = (cells + 1023) / 1024, c0 = per * threadIdx.x, c1 = c0 + per < cells ? c0 + per : cells;
    uint32_t sum = 0;
    for (int64_t c = c0; c < c1; ++c) sum += ws.count[c];
    uint32_t total;
    uint32_t run = block_exclusive_scan<1024>(sum, scratch, &total);
    for (int64_t c = c0; c < c1; ++c) {
        const uint32_t n = ws.count[c];
        ws.offsets[c] = run;
        ws.count[c] = 0;
        run += n;
    }
    if (threadIdx.x == 0) ws.offsets[cells] = total;
}

static __global__ __launch_bounds__(FIELD_WG) void field_scatter_kernel(DgsFieldArgs a, FieldWs ws) {
    const int i = blockIdx.x * FIELD_WG + threadIdx.x;
    if (i >= a.N) return;
    const uint32_t key = ws.keys[i];
    ws.index[ws.offsets[key] + atomicAdd(&ws.count[key], 1u)] = (uint32_t)i;
}

// Slot of Gaussian i among the sorted records: its cell's offset plus the number of smaller indices in the cell's segment.
__device__ __forceinline__ uint32_t field_slot(const FieldWs& ws, int i) {
    const uint32_t key = ws.keys[i], beg = ws.offsets[key], end = ws.offsets[key + 1];
    uint32_t rank = 0;
    for (uint32_t j = beg; j < end; ++j) rank += ws.index[j] < (uint32_t)i ? 1u : 0u;
    return beg + rank;
}

static __global__ __launch_bounds__(FIELD_WG) void field_prepare_kernel(DgsFieldArgs a, FieldWs ws) {
    const int i = blockIdx.x * FIELD_WG + threadIdx.x;
    if (i >= a.N) return;
    const uint32_t slot = field_slot(ws, i);
    // -1/2 Sigma^-1 = -1/2 R diag(1 / s^2) R^T, s = exp(scaling) * scaling_modifier * mesh_scale, R of the normalised quaternion
    const double mul = (double)a.scaling_modifier * (double)a.mesh_scale;
    double w[3];
    for (int k = 0; k < 3; ++k) {
        const double s = exp((double)a.scaling[3 * (size_t)i + k]) * mul;
        w[k] = -0.5 / (s * s);
    }
    double q[4];
    for (int k = 0; k < 4; ++k) q[k] = (double)a.rotation[4 * (size_t)i + k];
    const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double r = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)},
                            {2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)},
                            {2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)}};
    auto m = [&](int p, int q2) { return R[p][0] * R[q2][0] * w[0] + R[p][1] * R[q2][1] * w[1] + R[p][2] * R[q2][2] * w[2]; };
    const double op = 1.0 / (1.0 + exp(-(double)a.opacity[i]));
    // power = A dx^2 + D dy^2 + F dz^2 + B dx dy + C dx dz + E dy dz: the off-diagonal coefficients carry the factor 2
    float4* out = ws.rec + 3 * (size_t)slot;
    out[0] = make_float4(a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2], (float)op);
    out[1] = make_float4((float)m(0, 0), (float)(2 * m(0, 1)), (float)(2 * m(0, 2)), (float)m(1, 1));
    out[2] = make_float4((float)(2 * m(1, 2)), (float)m(2, 2), 0.f, 0.f);
}

// exp(power): 2^(power * log2 e) on the hardware's v_exp_f32 with the rounding error of the argument compensated (the form of
// dgs_device.h blend_exp, without its alpha cut-off band: nothing here is thresholded).
__device__ __forceinline__ float field_exp(float power) {
    const float kL2eHi = 1.44269504088896341f;
    const float kL2eLo = (float)(1.44269504088896341 - (double)1.44269504088896341f);
    const float t = power * kL2eHi;
    float e = __builtin_fmaf(power, kL2eHi, -t);
    e = __builtin_fmaf(power, kL2eLo, e);
    const float ex = hw_exp2(t);
    return __builtin_fmaf(ex, e * 0.693147180559945309f, ex);
}

// The four launches (after the memset of the counts) that sort the rows of a.xyz into their cells and write the Gaussians' records.
static inline bool field_bin_gaussians(const DgsFieldArgs& a, const FieldWs& ws, hipStream_t st) {
    const int64_t cells = (int64_t)a.nb * a.nb * a.nb;
    const dim3 per_gaussian((a.N + FIELD_WG - 1) / FIELD_WG);
    if (hipMemsetAsync(ws.count, 0, 4 * cells, st) != hipSuccess) return false;
    hipLaunchKernelGGL(field_key_kernel, per_gaussian, dim3(FIELD_WG), 0, st, a, ws);
    hipLaunchKernelGGL(field_scan_kernel, dim3(1), dim3(1024), 0, st, ws, cells);
    hipLaunchKernelGGL(field_scatter_kernel, per_gaussian, dim3(FIELD_WG), 0, st, a, ws);
    hipLaunchKernelGGL(field_prepare_kernel, per_gaussian, dim3(FIELD_WG), 0, st, a, ws);
    return true;
}

}  // namespace dgs
#endif
