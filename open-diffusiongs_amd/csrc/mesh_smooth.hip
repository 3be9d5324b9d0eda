// mesh_smooth.hip -- Taubin lambda | mu smoothing of a triangle mesh's vertices on the device (include/dgs_mesh_smooth.h
// DgsMeshSmoothArgs; the order-free counterpart of MeshLab's apply_coord_taubin_smoothing with the cotangent weights off, which the
// reference carries as the commented alternative of its remeshing).  The header holds the definition; this file is its kernel sequence.
//
// dgs_mesh_smooth (one memset: the zeroed arrays):
//   sm_count_kernel   thread = face: invalid and null faces counted (one atomic a wave, issued only by a wave that has some), and
//                     cnt[a]++, cnt[b]++, cnt[c]++ for the others.  The lanes of a wave that name the vertex its first active lane
//                     names add once, together (sm_wave_add): a fan of 10^6 faces on one hub is 15,625 adds on that word, not 10^6.
//   sm_scan_kernel    thread = vertex: the segment length (2 c_v for a moving vertex, 0 for every other: nothing reads their
//                     neighbours), exclusive scan over the workgroup, block totals aside; the vertices over the cap and the
//                     unreferenced ones counted per block in one packed word.
//   sm_sums_kernel    one workgroup: exclusive scan of the block totals, the packed words added up, the four counts to the caller.
//   sm_fill_kernel    thread = face: each corner that moves takes two entries of its segment through the vertex's cursor (atomicAdd of
//                     2, shared over the wave as in sm_count_kernel) and stores its two other corners there as one 8-byte vector store.
//                     The order inside a segment is the order of arrival; sm_pass_kernel adds integers, so its sums do not depend
//                     on it.
//   sm_pass_kernel    thread = vertex, once per pass with a weight other than 0: a pure gather from `src` to `dst`.  A moving vertex
//                     of c_v <= SM_THREAD_MAX walks its segment itself, a face's two entries a step.  Then the wave takes the moving
//                     vertices of its 64 with c_v > SM_THREAD_MAX one after another (a ballot; none on an ordinary mesh): the lanes
//                     stride over the segment,
//                     their int64 partial sums meet in an xor butterfly (integer adds: any tree gives the same bits), and the lane
//                     that owns the vertex keeps the sum.  Every lane then evaluates the header's fp64 expression for its own vertex,
//                     or copies the three words of a vertex that does not move.  The trip count of every loop is a segment length
//                     (over the lanes): 10^6 faces on one vertex cost what 10^6 faces cost, and that vertex, above the cap, has no
//                     segment at all.
// The passes go from `vertices` to the workspace's buffer and out_vertices in turn, so that the last one writes out_vertices; with no
// pass to run the input is copied.  The only atomics are the integer adds of the counters and the cursors; no kernel waits for another
// workgroup; same input, same bytes.  STRICT_FP (dgs_amd/build.py): no fused multiply-add, so numpy (tests/mesh_smooth_util.py) and the
// emulator build compute every position as the device does.  Every fp64 operand is converted from a per-lane load
// (csrc/mesh_clean.hip, clean_threshold_kernel, says why): the wave path hands the sum to the owning lane for that reason too.
//
// Workspace: 16 B a vertex (cnt, cursor, start, and a word per block), 12 B a vertex for the second buffer, 24 B a face for the
// neighbours.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "dgs_device.h"
#include "dgs_mesh_smooth.h"
#include "mesh_common.h"

namespace dgs {

constexpr int SM_WG = 256;
constexpr int64_t SM_MAX_V = (int64_t)1 << 30;
constexpr int64_t SM_MAX_F = (int64_t)1 << 29;        // 6 F < 2^32: positions in the neighbour array are uint32
constexpr int SM_MAX_ITERATIONS = 1 << 20;
constexpr uint32_t SM_CAP = 16384;                    // the header's incidence cap: 2^15 entries of 2^47 stay below 2^63
constexpr uint32_t SM_THREAD_MAX = 48;                // c_v <= 48: a thread walks the segment; above: a wave
constexpr double SM_ONE = 4294967296.0;               // 2^32: the fixed point of the sums
constexpr double SM_CLAMP = 32768.0;
enum { SM_INVALID = 0, SM_NULL = 1, SM_MISC_WORDS = 4 };

struct SmWs {
    uint32_t* misc;                                   // [SM_MISC_WORDS]
    uint32_t* cnt;                                    // [V] c_v
    uint32_t* cursor;                                 // [V] entries of the segment taken so far
    uint32_t* start;                                  // [V] the segment's start inside its block
    uint32_t* blk;                                    // [vblocks] entries of the block, then scanned
    uint32_t* flg;                                    // [vblocks] vertices over the cap (low half) and unreferenced (high half)
    float* tmp;                                       // [V, 3] the passes' second buffer
    int32_t* nbr;                                     // [6 F] the segments
    int64_t vblocks, fblocks, zero_bytes, bytes;
    __host__ SmWs(void* base, int64_t V, int64_t F) {
        MeshCarver c(base);                                              // base == nullptr: only the sizes are used
        vblocks = (V + SM_WG - 1) / SM_WG;
        fblocks = (F + SM_WG - 1) / SM_WG;
        misc = c.take<uint32_t>(SM_MISC_WORDS);                          // misc, cnt, cursor: zeroed by the call's one memset
        cnt = c.take<uint32_t>(V);
        cursor = c.take<uint32_t>(V);
        zero_bytes = c.used();
        start = c.take<uint32_t>(V);
        blk = c.take<uint32_t>(vblocks);
        flg = c.take<uint32_t>(vblocks);
        tmp = c.take<float>(3 * V);
        nbr = c.take<int32_t>(6 * F);
        bytes = c.used();
    }
};

__device__ __forceinline__ bool sm_moving(uint32_t c, const uint8_t* fixed, uint32_t v) {
    return c >= 1 && c <= SM_CAP && (fixed == nullptr || fixed[v] == 0);
}

// atomicAdd(p + idx, amount) of every active lane -> the value before this lane's add, as if the lanes came one after another.  The
// lanes that name the index of the first active lane add once, through that lane; the others add for themselves.  The whole wave calls.
__device__ __forceinline__ uint32_t sm_wave_add(uint32_t* p, bool active, uint32_t idx, uint32_t amount) {
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    const uint64_t act = wave_ballot(active);
    if (act == 0) return 0;                                               // the whole wave
    const int leader = __ffsll((long long)act) - 1;
    const uint32_t first = __shfl(idx, leader);
    const bool with = active && idx == first;
    const uint64_t same = wave_ballot(with);
    uint32_t got = 0;
    if (lane == leader) got = atomicAdd(p + first, (uint32_t)__popcll(same) * amount);
    got = __shfl(got, leader);
    if (with) return got + (uint32_t)__popcll(same & ((1ull << lane) - 1)) * amount;
    return active ? atomicAdd(p + idx, amount) : 0;
}

__global__ __launch_bounds__(SM_WG) void sm_count_kernel(DgsMeshSmoothArgs a, SmWs ws) {
    const uint32_t f = blockIdx.x * SM_WG + threadIdx.x, V = (uint32_t)a.V;
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    bool invalid = false, null = false, live = false;
    uint32_t t[3] = {0, 0, 0};
    if (f < (uint32_t)a.F) {
        const int32_t* in = a.faces + 3 * (size_t)f;
        const int i = in[0], j = in[1], k = in[2];
        invalid = !mesh_face_valid(i, j, k, V);
        null = !invalid && (i == j || i == k || j == k);
        live = !invalid && !null;
        t[0] = (uint32_t)i;
        t[1] = (uint32_t)j;
        t[2] = (uint32_t)k;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) sm_wave_add(ws.cnt, live, t[c], 1u);
    const uint64_t mi = wave_ballot(invalid), mn = wave_ballot(null);
    if (mi != 0 && lane == 0) atomicAdd(ws.misc + SM_INVALID, (uint32_t)__popcll(mi));
    if (mn != 0 && lane == 0) atomicAdd(ws.misc + SM_NULL, (uint32_t)__popcll(mn));
}

__global__ __launch_bounds__(SM_WG) void sm_scan_kernel(DgsMeshSmoothArgs a, SmWs ws) {
    __shared__ uint32_t scratch[SM_WG / DGS_WAVE + 1];
    const uint32_t v = blockIdx.x * SM_WG + threadIdx.x;
    const bool in = v < (uint32_t)a.V;
    const uint32_t c = in ? ws.cnt[v] : 0u;
    const uint32_t len = in && sm_moving(c, a.fixed, v) ? 2u * c : 0u;  // <= 2^15 a vertex, 2^23 a block
    uint32_t total, flags;
    const uint32_t before = block_exclusive_scan<SM_WG>(len, scratch, &total);
    block_exclusive_scan<SM_WG>((in && c > SM_CAP ? 1u : 0u) | (in && c == 0 ? 0x10000u : 0u), scratch, &flags);   // <= 256 in each half
    if (in) ws.start[v] = before;
    if (threadIdx.x == 0) {
        ws.blk[blockIdx.x] = total;
        ws.flg[blockIdx.x] = flags;
    }
}

// Exclusive scan of the block totals in place by one workgroup of 1,024 (the form of mesh_scan_blocks, csrc/mesh_common.h), the packed flags added up, the
// counts to the caller.
__global__ __launch_bounds__(1024) void sm_sums_kernel(DgsMeshSmoothArgs a, SmWs ws) {
    __shared__ uint32_t scratch[1024 / DGS_WAVE + 1];
    const int64_t n = ws.vblocks, per = (n + 1023) / 1024, c0 = per * threadIdx.x, c1 = c0 + per < n ? c0 + per : n;
    uint32_t s = 0, over = 0, unref = 0;
    for (int64_t c = c0; c < c1; ++c) {
        s += ws.blk[c];
        over += ws.flg[c] & 0xffffu;
        unref += ws.flg[c] >> 16;
    }
    uint32_t total, all_over, all_unref;
    uint32_t run = block_exclusive_scan<1024>(s, scratch, &total);
    block_exclusive_scan<1024>(over, scratch, &all_over);
    block_exclusive_scan<1024>(unref, scratch, &all_unref);
    for (int64_t c = c0; c < c1; ++c) {
        const uint32_t here = ws.blk[c];
        ws.blk[c] = run;
        run += here;
    }
    if (threadIdx.x == 0 && a.counts) {
        a.counts[0] = ws.misc[SM_INVALID];
        a.counts[1] = ws.misc[SM_NULL];
        a.counts[2] = all_over;
        a.counts[3] = all_unref;
    }
}

__global__ __launch_bounds__(SM_WG) void sm_fill_kernel(DgsMeshSmoothArgs a, SmWs ws) {
    const uint32_t f = blockIdx.x * SM_WG + threadIdx.x, V = (uint32_t)a.V;
    bool live = false;
    uint32_t t[3] = {0, 0, 0};
    if (f < (uint32_t)a.F) {
        const int32_t* in = a.faces + 3 * (size_t)f;
        const int i = in[0], j = in[1], k = in[2];
        live = mesh_face_valid(i, j, k, V) && i != j && i != k && j != k;
        t[0] = (uint32_t)i;
        t[1] = (uint32_t)j;
        t[2] = (uint32_t)k;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t x = t[c], len = live ? 2u * ws.cnt[x] : 0u;
        const bool moves = live && sm_moving(len >> 1, a.fixed, x);
        const uint32_t at = sm_wave_add(ws.cursor, moves, x, 2u);
        if (moves) {
            if (at + 2u <= len) {                                         // always (the faces counted are the faces filled); stay in range anyway
                const size_t pos = (size_t)ws.blk[x / SM_WG] + ws.start[x] + at;   // even: 8-byte aligned
                *reinterpret_cast<int2*>(ws.nbr + pos) = make_int2((int)t[(c + 1) % 3], (int)t[(c + 2) % 3]);
            }
        }
    }
}

// The header's Q.  |d * 2^32| <= 2^47, so adding 1.5 * 2^52 rounds it to an integer (to nearest, ties to even: what llrint does) that
// sits in the low bits of the sum's mantissa: two fp64 operations and an integer subtraction where the conversion to int64 takes a
// dozen.  A NaN gives some integer; no address depends on it.
__device__ __forceinline__ long long sm_fixed_point(float x) {
    constexpr double magic = 6755399441055744.0;                          // 1.5 * 2^52
    double d = (double)x;
    d = d < -SM_CLAMP ? -SM_CLAMP : d;
    d = d > SM_CLAMP ? SM_CLAMP : d;
    const double r = d * SM_ONE + magic;
    return __builtin_bit_cast(long long, r) - __builtin_bit_cast(long long, magic);
}

__global__ __launch_bounds__(SM_WG) void sm_pass_kernel(DgsMeshSmoothArgs a, SmWs ws, const float* __restrict__ src, float* __restrict__ dst, double w) {
    const uint32_t v = blockIdx.x * SM_WG + threadIdx.x;
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    const bool in = v < (uint32_t)a.V;
    const uint32_t c = in ? ws.cnt[v] : 0u;
    const bool moves = in && sm_moving(c, a.fixed, v);
    const uint32_t len = moves ? 2u * c : 0u;
    const size_t begin = moves ? (size_t)ws.blk[v / SM_WG] + ws.start[v] : 0;
    long long sum[3] = {0, 0, 0};
    if (moves && c <= SM_THREAD_MAX) {
        const int2* pair = reinterpret_cast<const int2*>(ws.nbr + begin); // a face's two other corners: six independent gathers a step
        for (uint32_t e = 0; e < c; ++e) {
            const int2 uv = pair[e];
            const float *q0 = src + 3 * (size_t)uv.x, *q1 = src + 3 * (size_t)uv.y;
            const float x0 = q0[0], y0 = q0[1], z0 = q0[2], x1 = q1[0], y1 = q1[1], z1 = q1[2];
            sum[0] += sm_fixed_point(x0) + sm_fixed_point(x1);
            sum[1] += sm_fixed_point(y0) + sm_fixed_point(y1);
            sum[2] += sm_fixed_point(z0) + sm_fixed_point(z1);
        }
    }
    uint64_t wide = wave_ballot(moves && c > SM_THREAD_MAX);
    while (wide != 0) {                                                   // the whole wave, one long segment after another
        const int owner = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const uint32_t n = __shfl(len, owner);
        const unsigned long long from = __shfl((unsigned long long)begin, owner);
        long long part[3] = {0, 0, 0};
        for (uint32_t e = (uint32_t)lane; e < n; e += DGS_WAVE) {
            const float* q = src + 3 * (size_t)ws.nbr[from + e];
#pragma unroll
            for (int k = 0; k < 3; ++k) part[k] += sm_fixed_point(q[k]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int d = 1; d < DGS_WAVE; d <<= 1) part[k] += __shfl_xor(part[k], d);
            if (lane == owner) sum[k] = part[k];
        }
    }
    if (!in) return;
    const float* p = src + 3 * (size_t)v;
    float* out = dst + 3 * (size_t)v;
    if (moves) {
        const double weight = (double)len * SM_ONE;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double here = (double)p[k];
            const double mean = (double)sum[k] / weight;                  // each operation rounded on its own: STRICT_FP
            const double step = w * (mean - here);
            out[k] = (float)(here + step);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = p[k];                        // the bytes: a load and a store, no arithmetic
    }
}

static bool sm_args_ok(const DgsMeshSmoothArgs* a) {
    if (!a || a->V < 0 || a->F < 0 || a->V > SM_MAX_V || a->F > SM_MAX_F || a->iterations < 0 || a->iterations > SM_MAX_ITERATIONS) return false;
    if (!(a->lambda - a->lambda == 0.0) || !(a->mu - a->mu == 0.0)) return false;                    // finite
    if ((a->V > 0 && (!a->vertices || !a->out_vertices)) || (a->F > 0 && !a->faces)) return false;
    if (a->V > 0) {
        const uintptr_t in = reinterpret_cast<uintptr_t>(a->vertices), out = reinterpret_cast<uintptr_t>(a->out_vertices), bytes = 12 * (uintptr_t)a->V;
        if (in < out + bytes && out < in + bytes) return false;
    }
    return a->workspace && (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0 && a->workspace_bytes >= SmWs(nullptr, a->V, a->F).bytes;
}

// V = 0: every face is invalid.  F = 0: every vertex is unreferenced.
__global__ void sm_nothing_kernel(uint32_t* counts, uint32_t invalid, uint32_t unreferenced) {
    if (threadIdx.x < 4) counts[threadIdx.x] = threadIdx.x == 0 ? invalid : threadIdx.x == 3 ? unreferenced : 0u;
}

}  // namespace dgs

extern "C" int64_t dgs_mesh_smooth_workspace_bytes(int64_t V, int64_t F) {
    if (V < 0 || F < 0 || V > dgs::SM_MAX_V || F > dgs::SM_MAX_F) return 0;
    return dgs::SmWs(nullptr, V, F).bytes;
}

extern "C" int dgs_mesh_smooth(const DgsMeshSmoothArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!sm_args_ok(a)) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SmWs ws(a->workspace, a->V, a->F);
    const dim3 wg(SM_WG), vgrid((unsigned)ws.vblocks), fgrid((unsigned)ws.fblocks);
    const double weights[2] = {a->lambda, a->mu};
    const int per = (weights[0] != 0.0 ? 1 : 0) + (weights[1] != 0.0 ? 1 : 0);
    const int64_t passes = a->V > 0 && a->F > 0 ? (int64_t)a->iterations * per : 0;   // without a face nothing moves
    if (a->V == 0 || a->F == 0) {
        if (a->counts) hipLaunchKernelGGL(sm_nothing_kernel, dim3(1), dim3(DGS_WAVE), 0, st, a->counts, (uint32_t)(a->V == 0 ? a->F : 0), (uint32_t)(a->V == 0 ? 0 : a->V));
    } else {
        if (hipMemsetAsync(ws.misc, 0, (size_t)ws.zero_bytes, st) != hipSuccess) return DGS_ERR_DEVICE;
        hipLaunchKernelGGL(sm_count_kernel, fgrid, wg, 0, st, *a, ws);
        hipLaunchKernelGGL(sm_scan_kernel, vgrid, wg, 0, st, *a, ws);
        hipLaunchKernelGGL(sm_sums_kernel, dim3(1), dim3(1024), 0, st, *a, ws);
        if (passes > 0) hipLaunchKernelGGL(sm_fill_kernel, fgrid, wg, 0, st, *a, ws);
    }
    if (passes == 0) {
        if (a->V > 0 && hipMemcpyAsync(a->out_vertices, a->vertices, 12 * (size_t)a->V, hipMemcpyDeviceToDevice, st) != hipSuccess) return DGS_ERR_DEVICE;
        return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
    }
    const float* src = a->vertices;
    int64_t left = passes;
    for (int it = 0; it < a->iterations; ++it) {
        for (int s = 0; s < 2; ++s) {
            if (weights[s] == 0.0) continue;
            --left;
            float* dst = (left & 1) ? ws.tmp : a->out_vertices;          // the last pass (left == 0) writes out_vertices
            hipLaunchKernelGGL(sm_pass_kernel, vgrid, wg, 0, st, *a, ws, src, dst, weights[s]);
            src = dst;
        }
    }
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
