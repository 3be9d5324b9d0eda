// field.hip -- the Gaussian density field on a voxel grid (include/dgs_field.h DgsFieldArgs; the reference's
// GaussianModel.extract_fields, diffusionGS/models/gsrenderer/gs_core.py:786-852, a host loop over num_blocks^3 blocks).
//
// Five launches and one memset per call, all on the caller's stream (the first four live in field_cells.h, shared with mesh_attr.hip):
//   field_key_kernel      thread = Gaussian: the coarse cell (pitch block_size = 2 / nb) of its normalised centre, counted per cell
//   field_scan_kernel     one workgroup: exclusive scan of the nb^3 counts -> cell offsets; the counts become the scatter's cursors
//   field_scatter_kernel  thread = Gaussian: its index into its cell's segment, at whatever slot the atomic hands out
//   field_prepare_kernel  thread = Gaussian: its rank = the number of smaller indices in its cell's segment (so the order inside a cell
//                         is the index order, whatever the atomics did), then its record at offset + rank: centre, sigmoid(opacity)
//                         and the six coefficients of -1/2 Sigma^-1, Sigma^-1 = R diag(1 / s^2) R^T, evaluated in fp64 and rounded
//                         once (N threads of a few hundred operations: not worth saving; the records are then exact to 1/2 ulp)
//   field_eval_kernel     a workgroup of 256 threads per task.  split <= 4 (the pipeline's 256 / 64): four z-adjacent blocks, one wave
//                         each, lane = voxel.  split > 4: one block, 1024 voxels per pass (four per thread), ceil(split^3 / 1024) passes
//                         as workgroups of their own.  The workgroup walks the cells its blocks' member boxes can overlap -- the cell
//                         function is monotone, so they are the cells from cell(lo) to cell(hi), evaluated by the same device
//                         function that binned the centres -- one (cx, cy) row of z-adjacent cells at a time (their records are
//                         contiguous), 256 records per LDS stage; the staging thread tests x and y membership once for all lanes.
//                         Every lane reads the same record (LDS broadcast), the exact membership test compares the fp32 numbers
//                         the caller formed and is uniform over the wave; members accumulate in staging order with plain adds, the
//                         voxel is written with a plain store.  Non-members (~60 % of the staged records: the 5^3 cells cover 125
//                         block_size^3, the member box 3.75^3 = 53) cost one LDS read and a branch.
// Four z-adjacent blocks walk 8 cells of each of the 5 x 5 rows where four workgroups of one block would walk 4 x 5: 2.5 times fewer
// staged bytes.
// exp(power): 2^(power * log2 e) on the hardware's v_exp_f32 with the rounding error of the argument compensated (the form of
// dgs_device.h blend_exp, without its alpha cut-off band: nothing here is thresholded).
//
// Traffic and arithmetic at the pipeline's setting R = 256, nb = 64, N = 262,144 on a shell (tools/field_bench.py, profiles/field_bench.json,
// profiles/field_kernel_stats.txt; one MI355X):
//   bytes      occ 67 MB written once; records 48 B x N = 12.6 MB written once and staged by the ~5^3 / 4 workgroups around them (L2 hits);
//              inputs 11.5 MB, keys / indices 4 MB, counts + offsets 3 MB: 111 MB that must move.
//   arithmetic per (voxel, member) pair: 3 sub, 9 mul / fma of the quadratic form, 7 of the exponential, max, compare + select,
//              1 mul, 1 add = 23 VALU lane operations; 8.76e8 pairs (counted from the member boxes).
//   measured   field_eval_kernel 2.28 ms (0.76 ms at R = 128, nb = 32, N = 65,536), field_scan_kernel 0.55 ms (0.07), prepare 33 us,
//              scatter 28 us, key 27 us; the whole extract_fields call 3.4 ms (1.4 ms) against 148 s (18-23 s) for the block loop
//              written with torch ops.  The eval kernel runs 3.8e11 pairs/s = 0.11 of the fp32 VALU peak, and the call moves its
//              111 MB at 0.005 of the copy bandwidth: bound by neither.  What holds the eval kernel is the walk itself (an LDS
//              read and a branch for every staged non-member, two barriers per stage of at most 256 records, workgroups with very
//              uneven work: a block has between 0 and ~1,400 members); the single-workgroup scan of 262,144 counts is a sixth of the call.
//              Both are the next things to take; neither changes a result.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): field_eval_kernel<true> 30 VGPRs, <false> 58 VGPRs,
//   12,288 B LDS; prepare 44 VGPRs (fp64), scan 28, key / scatter 8.
// Deterministic: per-cell order = index order, cells in a fixed walk, one accumulator per voxel.
// STRICT_FP (dgs_amd/build.py): nothing is fused that is not written as fmaf, so the emulator build rounds like the device except inside 2^x.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "dgs_device.h"
#include "dgs_field.h"
#include "field_cells.h"     // FieldWs, field_cell, the key / scan / scatter / prepare kernels, field_exp

namespace dgs {

constexpr int FIELD_VPT = 4;         // voxels per thread and pass when split > 4
constexpr int FIELD_ZB = 4;          // z-adjacent blocks per workgroup when split <= 4
constexpr int FIELD_MAX_R = 2048;

// WAVE_PER_BLOCK: grid (ceil(nb / 4), nb, nb), wave w owns block (blockIdx.z, blockIdx.y, 4 blockIdx.x + w), lane = voxel (split^3 <= 64).
// otherwise:      grid (nb * passes, nb, nb), the workgroup owns voxels [1024 pass, 1024 (pass + 1)) of block (blockIdx.z, blockIdx.y, blockIdx.x / passes).
template <bool WAVE_PER_BLOCK>
__global__ __launch_bounds__(FIELD_WG) void field_eval_kernel(DgsFieldArgs a, FieldWs ws, int passes) {
    __shared__ __attribute__((aligned(16))) float4 srec[3 * FIELD_WG];
    constexpr int VPT = WAVE_PER_BLOCK ? 1 : FIELD_VPT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nb = a.nb, s = a.split, s3 = s * s * s;
    const int xi = blockIdx.z, yi = blockIdx.y;
    const int zfirst = WAVE_PER_BLOCK ? (int)blockIdx.x * FIELD_ZB : (int)blockIdx.x / passes;
    const int zlast = WAVE_PER_BLOCK ? (zfirst + FIELD_ZB - 1 < nb ? zfirst + FIELD_ZB - 1 : nb - 1) : zfirst;
    const int pass = WAVE_PER_BLOCK ? 0 : (int)blockIdx.x - zfirst * passes;
    const int zi = WAVE_PER_BLOCK ? zfirst + wave : zfirst;
    const bool live = zi < nb;                                  // a wave past the last block still stages and keeps the barriers
    const int zic = live ? zi : nb - 1;
    const float lox = a.lo[xi], hix = a.hi[xi], loy = a.lo[yi], hiy = a.hi[yi], loz = a.lo[zic], hiz = a.hi[zic];
    const int nv = WAVE_PER_BLOCK ? 1 : (s3 - pass * FIELD_WG * VPT + FIELD_WG - 1) / FIELD_WG;     // voxel slots of this pass in use (uniform)

    float vx[VPT], vy[VPT], vz[VPT], acc[VPT];
    size_t at[VPT];
    bool ok[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int idx = WAVE_PER_BLOCK ? lane : (pass * VPT + v) * FIELD_WG + tid;
        ok[v] = live && idx < s3;
        const int id = ok[v] ? idx : 0;
        const int ix = id / (s * s), iy = (id / s) % s, iz = id % s;
        const int gx = xi * s + ix, gy = yi * s + iy, gz = zic * s + iz;
        vx[v] = a.lin[gx];
        vy[v] = a.lin[gy];
        vz[v] = a.lin[gz];
        at[v] = ((size_t)gx * a.R + gy) * a.R + gz;
        acc[v] = 0.f;
    }

    const int cx0 = field_cell(lox, nb), cx1 = field_cell(hix, nb), cy0 = field_cell(loy, nb), cy1 = field_cell(hiy, nb);
    const int cz0 = field_cell(a.lo[zfirst], nb), cz1 = field_cell(a.hi[zlast], nb);
    for (int cx = cx0; cx <= cx1; ++cx)
        for (int cy = cy0; cy <= cy1; ++cy) {
            const size_t row = ((size_t)cx * nb + cy) * nb;
            const uint32_t beg = ws.offsets[row + cz0], end = ws.offsets[row + cz1 + 1];
            for (uint32_t base = beg; base < end; base += FIELD_WG) {
                const int n = end - base < (uint32_t)FIELD_WG ? (int)(end - base) : FIELD_WG;
                __syncthreads();                                 // the previous stage has been read by every wave
                if (tid < n) {
                    const float4* g = ws.rec + 3 * (size_t)(base + tid);
                    const float4 r0 = g[0], r1 = g[1];
                    float4 r2 = g[2];
                    r2.z = (lox < r0.x && r0.x < hix && loy < r0.y && r0.y < hiy) ? 1.f : 0.f;
                    srec[3 * tid] = r0;
                    srec[3 * tid + 1] = r1;
                    srec[3 * tid + 2] = r2;
                }
                __syncthreads();
                for (int j = 0; j < n; ++j) {
                    const float4 r0 = srec[3 * j], r2 = srec[3 * j + 2];
                    if (!(r2.z != 0.f && loz < r0.z && r0.z < hiz)) continue;           // uniform over the wave
                    const float4 r1 = srec[3 * j + 1];
#pragma unroll
                    for (int v = 0; v < VPT; ++v) {
                        if (v >= nv) continue;                                            // uniform over the workgroup
                        const float dx = vx[v] - r0.x, dy = vy[v] - r0.y, dz = vz[v] - r0.z;
                        const float px = __builtin_fmaf(r1.x, dx, __builtin_fmaf(r1.y, dy, r1.z * dz));
                        const float py = __builtin_fmaf(r1.w, dy, r2.x * dz);
                        const float power = __builtin_fmaf(dx, px, __builtin_fmaf(dy, py, (r2.y * dz) * dz));
                        // the reference's rule: a positive power is weight 0.  Below -126 the weight is under 2^-181: 0 in fp32 anyway
                        const float wgt = (power > 0.f) ? 0.f : field_exp(fmaxf(power, -126.0f));
                        acc[v] = acc[v] + r0.w * wgt;
                    }
                }
            }
        }
#pragma unroll
    for (int v = 0; v < VPT; ++v)
        if (ok[v]) a.occ[at[v]] = acc[v];
}

static bool field_args_ok(const DgsFieldArgs* a) {
    return a && a->N >= 1 && a->nb >= 1 && a->nb <= FIELD_MAX_NB && a->split >= 1 && a->split <= 1024 && a->R <= FIELD_MAX_R && (int64_t)a->nb * a->split == a->R &&
           a->xyz && a->scaling && a->rotation && a->opacity && a->lin && a->lo && a->hi && a->occ && a->workspace &&
           ((uintptr_t)a->workspace & 15) == 0;
}

}  // namespace dgs

extern "C" int64_t dgs_gaussian_field_workspace_bytes(int32_t N, int32_t nb) {
    if (N < 1 || nb < 1 || nb > dgs::FIELD_MAX_NB) return 0;
    return dgs::FieldWs(nullptr, N, nb).bytes;
}

extern "C" int dgs_gaussian_field(const DgsFieldArgs* a, dgs_stream_t stream) {
    if (!dgs::field_args_ok(a)) return DGS_ERR_INVALID_ARGUMENT;
    const dgs::FieldWs ws(a->workspace, a->N, a->nb);
    if (a->workspace_bytes < ws.bytes) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!dgs::field_bin_gaussians(*a, ws, st)) return DGS_ERR_DEVICE;
    const int s3 = a->split * a->split * a->split;
    if (a->split <= 4) {
        const dim3 grid((a->nb + dgs::FIELD_ZB - 1) / dgs::FIELD_ZB, a->nb, a->nb);
        hipLaunchKernelGGL(dgs::field_eval_kernel<true>, grid, dim3(dgs::FIELD_WG), 0, st, *a, ws, 1);
    } else {
        const int per_pass = dgs::FIELD_WG * dgs::FIELD_VPT, passes = (s3 + per_pass - 1) / per_pass;
        const dim3 grid(a->nb * passes, a->nb, a->nb);
        hipLaunchKernelGGL(dgs::field_eval_kernel<false>, grid, dim3(dgs::FIELD_WG), 0, st, *a, ws, passes);
    }
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
