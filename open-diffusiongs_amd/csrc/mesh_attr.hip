// mesh_attr.hip -- density, density gradient and density-weighted attribute (colour) of the Gaussians at query points: the vertex
// colours and shading normals of the mesh extract_mesh cuts from the density field (include/dgs_mesh_attr.h states the definition).
//
// Nine launches and two memsets per call, all on the caller's stream:
//   field_key / scan / scatter / prepare   field_cells.h, exactly as dgs_gaussian_field runs them: the Gaussians' 48-byte records sorted
//                                          by cell (pitch 2 / nb), in index order inside a cell
//   mesh_attr_gather_kernel                thread = Gaussian: its attribute as one float4 at the slot of its record (an array of its
//                                          own: the record and the field's LDS stage keep their size)
//   field_key / scan / scatter             the same three kernels on the query points (a second FieldWs names the points' arrays):
//                                          the points of a cell are contiguous in p.index, in whatever order the atomics left --
//                                          every point owns its accumulators, so that order reaches no output
//   mesh_attr_eval_kernel                  a workgroup of 256 threads per run of 4 z-adjacent point cells (their points are contiguous),
//                                          lane = point, ceil(points / 256) passes where a run holds more.  It walks the
//                                          (2 reach + 1)^2 rows of Gaussian cells around the run in ascending (cx, cy), a row's
//                                          cells z0 - reach .. z1 + reach being contiguous records, 256 records and attributes per
//                                          LDS stage (64 B each); the staging thread leaves the record's z cell in the record's spare
//                                          word.  Every lane reads the same record (LDS broadcast); |cz - cell(p_z)| <= reach is an
//                                          integer compare per lane; members accumulate in staging order = the header's order into
//                                          seven accumulators with plain adds; plain stores at the point's own index.  A run without
//                                          points returns before its first barrier.
// No workgroup waits for another; every loop's bound is read before the loop starts.
// Arithmetic per (point, member) pair: 3 sub, 9 mul / fma of the quadratic form, 9 of its gradient, 7 of the exponential, max,
//   compare + select, 1 mul (t), 6 mul + 7 add of the accumulators = 45 VALU lane operations; a staged non-member costs one LDS read,
//   an integer subtract, an absolute value and a compare.
// Measured at the pipeline's setting R = 256, nb = 64, N = 262,144, reach = 2 on the bench's shell scene (tools/mesh_attr_bench.py,
//   profiles/mesh_attr_bench.json, profiles/mesh_attr_kernel_stats.txt; one MI355X): the whole mesh_attributes call 2.20 ms at
//   V = 783,168 and 2.12 ms at V = 48,675 (1.34 / 1.12 ms at R = 128, nb = 32, N = 65,536, V = 500,537 / 43,736), against 21.83 s / 1.36 s
//   for the dense torch form.  Kernels: field_scan_kernel 549 us, twice a call (Gaussians, points) = half the call; mesh_attr_eval_kernel
//   382 us at either V; gather 26 us, prepare 31 us, key / scatter 5-42 us.  On that scene the level set lies four to five cells off
//   the shell, so a point has 9 members on average (6.97e6 pairs): the eval kernel's time is its 65,536 workgroups reading two offsets
//   each and the walk's barriers, not arithmetic (0.002 of the fp32 VALU peak over the call).  Bound by the single-workgroup scan first;
//   a scan over several workgroups and a launch over the occupied runs only are the next things to take, neither changes a result.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): mesh_attr_eval_kernel 40 VGPRs, 16,384 B LDS, scratch 0, 8 waves / SIMD;
//   mesh_attr_gather_kernel 18 VGPRs; the shared kernels as in field.hip (prepare 43 VGPRs, scan 28, key / scatter 8); scratch 0 everywhere.
// Deterministic: per-cell order = index order, cells in a fixed walk, one accumulator per output component.
// STRICT_FP (dgs_amd/build.py): nothing is fused that is not written as fmaf, so the emulator build rounds like the device except inside 2^x.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "dgs_device.h"
#include "dgs_mesh_attr.h"
#include "field_cells.h"

namespace dgs {

constexpr int ATTR_ZB = 4;           // z-adjacent point cells per workgroup
constexpr int ATTR_MAX_REACH = 8;
constexpr int64_t ATTR_MAX_V = (int64_t)1 << 30;

struct AttrWs {
    FieldWs g, p;                    // the Gaussians' binning and records; the points' binning (p.rec unused)
    float4* sattr;                   // [N] the attribute, sorted with the records
    int64_t bytes;
    __host__ AttrWs(void* base, int64_t N, int64_t nb, int64_t V) : g(base, N, nb), p(base, N, nb) {
        const int64_t cells = nb * nb * nb;
        auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
        char* b = static_cast<char*>(base);
        int64_t at = g.bytes;
        sattr = reinterpret_cast<float4*>(b + at);       at += 16 * N;
        p.count = reinterpret_cast<uint32_t*>(b + at);   at += up(4 * cells);
        p.offsets = reinterpret_cast<uint32_t*>(b + at); at += up(4 * (cells + 1));
        p.keys = reinterpret_cast<uint32_t*>(b + at);    at += up(4 * V);
        p.index = reinterpret_cast<uint32_t*>(b + at);   at += up(4 * V);
        p.rec = nullptr;
        p.bytes = 0;
        bytes = at;
    }
};

__global__ __launch_bounds__(FIELD_WG) void mesh_attr_gather_kernel(DgsMeshAttrArgs a, FieldWs g, float4* sattr) {
    const int i = blockIdx.x * FIELD_WG + threadIdx.x;
    if (i >= a.N) return;
    sattr[field_slot(g, i)] = make_float4(a.attr[3 * (size_t)i], a.attr[3 * (size_t)i + 1], a.attr[3 * (size_t)i + 2], 0.f);
}

// grid (ceil(nb / ATTR_ZB), nb, nb): the workgroup owns the points of cells (blockIdx.z, blockIdx.y, ATTR_ZB blockIdx.x .. + ATTR_ZB - 1)
__global__ __launch_bounds__(FIELD_WG) void mesh_attr_eval_kernel(DgsMeshAttrArgs a, FieldWs g, FieldWs p, const float4* sattr) {
    __shared__ __attribute__((aligned(16))) float4 srec[4 * FIELD_WG];
    const int tid = threadIdx.x, nb = a.nb, reach = a.reach;
    const int cx = blockIdx.z, cy = blockIdx.y, z0 = (int)blockIdx.x * ATTR_ZB, z1 = z0 + ATTR_ZB - 1 < nb ? z0 + ATTR_ZB - 1 : nb - 1;
    const size_t prow = ((size_t)cx * nb + cy) * nb;
    const uint32_t pbeg = p.offsets[prow + z0], pend = p.offsets[prow + z1 + 1];
    if (pbeg == pend) return;                                    // uniform: no point in the run, no barrier met
    const int gx0 = cx - reach > 0 ? cx - reach : 0, gx1 = cx + reach < nb - 1 ? cx + reach : nb - 1;
    const int gy0 = cy - reach > 0 ? cy - reach : 0, gy1 = cy + reach < nb - 1 ? cy + reach : nb - 1;
    const int gz0 = z0 - reach > 0 ? z0 - reach : 0, gz1 = z1 + reach < nb - 1 ? z1 + reach : nb - 1;
    const uint32_t passes = (pend - pbeg + FIELD_WG - 1) / FIELD_WG;
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t slot = pbeg + pass * FIELD_WG + tid;
        const bool ok = slot < pend;
        const uint32_t v = ok ? p.index[slot] : 0u;
        float px = 0.f, py = 0.f, pz = 0.f;
        int pcz = -4 * FIELD_MAX_NB;                             // a lane without a point is a member of nothing
        if (ok) {
            px = a.points[3 * (size_t)v];
            py = a.points[3 * (size_t)v + 1];
            pz = a.points[3 * (size_t)v + 2];
            pcz = field_cell(pz, nb);
        }
        float den = 0.f, ax = 0.f, ay = 0.f, az = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
        for (int rx = gx0; rx <= gx1; ++rx)
            for (int ry = gy0; ry <= gy1; ++ry) {
                const size_t row = ((size_t)rx * nb + ry) * nb;
                const uint32_t beg = g.offsets[row + gz0], end = g.offsets[row + gz1 + 1];
                for (uint32_t base = beg; base < end; base += FIELD_WG) {
                    const int n = end - base < (uint32_t)FIELD_WG ? (int)(end - base) : FIELD_WG;
                    __syncthreads();                             // the previous stage has been read by every wave
                    if (tid < n) {
                        const float4* r = g.rec + 3 * (size_t)(base + tid);
                        const float4 r0 = r[0], r1 = r[1];
                        float4 r2 = r[2];
                        r2.z = __int_as_float(field_cell(r0.z, nb));     // the cell the key kernel gave it, as bits
                        srec[4 * tid] = r0;
                        srec[4 * tid + 1] = r1;
                        srec[4 * tid + 2] = r2;
                        srec[4 * tid + 3] = sattr[base + tid];
                    }
                    __syncthreads();
                    for (int j = 0; j < n; ++j) {
                        const float4 r2 = srec[4 * j + 2];
                        const int dcz = __float_as_int(r2.z) - pcz;
                        if ((dcz < 0 ? -dcz : dcz) > reach) continue;
                        const float4 r0 = srec[4 * j], r1 = srec[4 * j + 1], at = srec[4 * j + 3];
                        const float dx = px - r0.x, dy = py - r0.y, dz = pz - r0.z;
                        const float qx = __builtin_fmaf(r1.x, dx, __builtin_fmaf(r1.y, dy, r1.z * dz));
                        const float qy = __builtin_fmaf(r1.w, dy, r2.x * dz);
                        const float power = __builtin_fmaf(dx, qx, __builtin_fmaf(dy, qy, (r2.y * dz) * dz));
                        const float wgt = (power > 0.f) ? 0.f : field_exp(fmaxf(power, -126.0f));
                        const float t = r0.w * wgt;
                        const float dpx = __builtin_fmaf(2.f * r1.x, dx, __builtin_fmaf(r1.y, dy, r1.z * dz));
                        const float dpy = __builtin_fmaf(r1.y, dx, __builtin_fmaf(2.f * r1.w, dy, r2.x * dz));
                        const float dpz = __builtin_fmaf(r1.z, dx, __builtin_fmaf(r2.x, dy, (2.f * r2.y) * dz));
                        den = den + t;
                        ax = ax + t * at.x;
                        ay = ay + t * at.y;
                        az = az + t * at.z;
                        gx = gx + t * dpx;
                        gy = gy + t * dpy;
                        gz = gz + t * dpz;
                    }
                }
            }
        if (ok) {
            if (a.density) a.density[v] = den;
            if (a.attr_out) {
                const bool some = den > 0.f;
                a.attr_out[3 * (size_t)v] = some ? ax / den : 0.f;
                a.attr_out[3 * (size_t)v + 1] = some ? ay / den : 0.f;
                a.attr_out[3 * (size_t)v + 2] = some ? az / den : 0.f;
            }
            if (a.gradient) {
                a.gradient[3 * (size_t)v] = gx;
                a.gradient[3 * (size_t)v + 1] = gy;
                a.gradient[3 * (size_t)v + 2] = gz;
            }
        }
    }
}

static bool mesh_attr_limits_ok(const DgsMeshAttrArgs* a) {
    return a && a->N >= 1 && a->nb >= 1 && a->nb <= FIELD_MAX_NB && a->reach >= 0 && a->reach <= ATTR_MAX_REACH && a->V >= 0 && a->V <= ATTR_MAX_V;
}

}  // namespace dgs

extern "C" int64_t dgs_mesh_attributes_workspace_bytes(int32_t N, int32_t nb, int64_t V) {
    if (N < 1 || nb < 1 || nb > dgs::FIELD_MAX_NB || V < 0 || V > dgs::ATTR_MAX_V) return 0;
    return dgs::AttrWs(nullptr, N, nb, V).bytes;
}

extern "C" int dgs_mesh_attributes(const DgsMeshAttrArgs* a, dgs_stream_t stream) {
    if (!dgs::mesh_attr_limits_ok(a)) return DGS_ERR_INVALID_ARGUMENT;
    if (a->V == 0) return DGS_OK;
    if (!(a->xyz && a->scaling && a->rotation && a->opacity && a->attr && a->points && a->workspace) || !(a->density || a->attr_out || a->gradient) ||
        ((uintptr_t)a->workspace & 15) != 0)
        return DGS_ERR_INVALID_ARGUMENT;
    const dgs::AttrWs ws(a->workspace, a->N, a->nb, a->V);
    if (a->workspace_bytes < ws.bytes) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DgsFieldArgs f = {};                                         // what the shared kernels read of it
    f.N = a->N;
    f.nb = a->nb;
    f.xyz = a->xyz;
    f.scaling = a->scaling;
    f.rotation = a->rotation;
    f.opacity = a->opacity;
    f.mesh_scale = a->mesh_scale;
    f.scaling_modifier = a->scaling_modifier;
    if (!dgs::field_bin_gaussians(f, ws.g, st)) return DGS_ERR_DEVICE;
    hipLaunchKernelGGL(dgs::mesh_attr_gather_kernel, dim3((a->N + dgs::FIELD_WG - 1) / dgs::FIELD_WG), dim3(dgs::FIELD_WG), 0, st, *a, ws.g, ws.sattr);
    DgsFieldArgs q = {};                                         // the points through the same key / scan / scatter
    q.N = (int32_t)a->V;
    q.nb = a->nb;
    q.xyz = a->points;
    const int64_t cells = (int64_t)a->nb * a->nb * a->nb;
    const dim3 per_point((unsigned)((a->V + dgs::FIELD_WG - 1) / dgs::FIELD_WG));
    if (hipMemsetAsync(ws.p.count, 0, 4 * cells, st) != hipSuccess) return DGS_ERR_DEVICE;
    hipLaunchKernelGGL(dgs::field_key_kernel, per_point, dim3(dgs::FIELD_WG), 0, st, q, ws.p);
    hipLaunchKernelGGL(dgs::field_scan_kernel, dim3(1), dim3(1024), 0, st, ws.p, cells);
    hipLaunchKernelGGL(dgs::field_scatter_kernel, per_point, dim3(dgs::FIELD_WG), 0, st, q, ws.p);
    const dim3 grid((a->nb + dgs::ATTR_ZB - 1) / dgs::ATTR_ZB, a->nb, a->nb);
    hipLaunchKernelGGL(dgs::mesh_attr_eval_kernel, grid, dim3(dgs::FIELD_WG), 0, st, *a, ws.g, ws.p, ws.sattr);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
