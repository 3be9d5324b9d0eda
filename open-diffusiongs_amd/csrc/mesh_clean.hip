// mesh_clean.hip -- drop the small connected components of a triangle mesh on the device (include/dgs_mesh_clean.h DgsMeshCleanArgs;
// replaces the two floater filters of the reference's clean_mesh, remove_connected_component_by_diameter / _by_face_number, and the
// remove_unreferenced_vertices that follows each).  The header holds the definition; this file is its kernel sequence.
//
// dgs_mesh_clean_count:
//   clean_init_kernel     thread = vertex: link[v] = v, ref / cnt / box of v cleared.
//   clean_link_kernel     thread = face: validity (invalid faces counted), ref[a] = ref[b] = ref[c] = 1, and atomicMin of each vertex's link
//                         to the face's smallest index: a forest inside the components.  It loses edges; the hook launch takes all again.
//   clean_compress_kernel thread = vertex, its own launch (nothing writes link[], plain loads): parent[v] = the root of v's link tree.
//   clean_hook_kernel     thread = face: union(a, b), union(a, c) in the lock-free union-find of csrc/mesh_common.h over the vertex indices
//                         (the root of a tree is the smallest index of its set; every access to parent[] in this launch is an agent-scope
//                         atomic), started from the three parents and skipped when those are equal already, which after the two launches
//                         before holds for nearly every face (hooking from parent[v] = v took 1.35 ms at 2.09 M faces, this form
//                         0.07 + 0.04 + 0.58 ms).
//   clean_flatten_kernel  thread = vertex, the next launch (plain loads now see the final links): lab[v] = root of v = canonical label.
//   clean_faces_kernel    lane = face: cnt[lab] += 1.  The lanes of a wave that share the leading lane's label add their number together
//                         (two rounds, whatever is left goes alone), the sums go to a 256-slot table of the workgroup in LDS, and the
//                         table is added to memory once per 4,096 faces: the giant component's 2 M adds would otherwise land on one
//                         counter, and the atomics of one address are served one after another (one per wave took 1.1 ms at 2.09 M
//                         faces).  The marching-cubes order interleaves the object's faces with the floaters', so runs of one label
//                         are short and a table is needed, not a run carried in registers (that form still took 0.88 ms).
//   clean_box_kernel      thread = vertex: atomicMax of the referenced vertices' coordinates into box[lab] and the mesh's box, as the
//                         order-preserving uint32 image of the floats (the minima stored complemented, so that zero is the identity of all
//                         six), combined per label inside the wave the same way, and only issued when the word read first is lower.
//   clean_threshold_kernel  one wave: (p * p) * D2 in fp64 from the mesh's box (only when the diameter rule is on).
//   clean_decide_kernel   thread = vertex; a root with cnt > 0 is a component: n and d2 (fp64) against the thresholds, keep[root], the
//                         two component counters.
//   clean_vscan_kernel    thread = vertex: flag = ref && keep[lab], exclusive scan over the workgroup, block totals aside.
//   clean_fscan_kernel    thread = face: flag = valid && keep[lab of its first index], likewise.
//   clean_sums_kernel     one workgroup: exclusive scan of both lists of block totals (the form of mesh_sums_kernel), counts to the caller.
// dgs_mesh_clean_emit:
//   clean_emit_vertices_kernel / clean_emit_faces_kernel   a flagged row goes to block base + offset when that is inside the caller's
//                         maximum; face indices are renumbered with the vertex offsets; labels (optional) for every input face.
// The only atomics are the union-find, the integer adds and the minima / maxima; positions come from the scans.  Same input, same bytes.
// STRICT_FP (dgs_amd/build.py): d2 = (dx * dx + dy * dy) + dz * dz is five fp64 roundings, never a fused multiply-add, so numpy
// (tests/mesh_clean_util.py) and the emulator build decide every component as the device does.
//
// Workspace: 52 B a vertex (link, parent, lab, ref, cnt, keep, scan offset 4 B each, box 24 B) + 4 B a face + 8 B per 256 of either + 64 B:
// 63 MB at the pipeline's setting (1.05 M vertices, 2.09 M faces).
// Measured on one MI355X: tools/mesh_clean_bench.py, profiles/mesh_clean_bench.json, profiles/mesh_clean_kernel_stats.txt.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dgs_device.h"
#include "dgs_mesh_clean.h"
#include "mesh_common.h"

namespace dgs {

constexpr int CLEAN_WG = 256;
constexpr int64_t CLEAN_MAX_ROWS = (int64_t)1 << 30;
constexpr int CLEAN_FACE_CHUNKS = 16;               // chunks of 64 faces a wave of clean_faces_kernel takes
constexpr int CLEAN_TALLY_BITS = 8;                 // 256 slots in clean_faces_kernel's table
constexpr uint32_t CLEAN_NO_LABEL = 0xffffffffu;     // no vertex index: V <= 2^30
constexpr int CLEAN_ROUNDS = 2;                      // labels a wave combines before the lanes left over add for themselves
enum { CLEAN_BOX = 0, CLEAN_COMPONENTS = 6, CLEAN_KEPT = 7, CLEAN_INVALID = 8, CLEAN_THRESHOLD = 10 /* a double */, CLEAN_MISC_WORDS = 16 };

struct CleanWs {
    uint32_t *link, *parent, *lab, *ref, *cnt, *keep; // [V]; cnt, keep: meaningful at roots
    uint32_t* box;                                   // [V, 6] at roots: ~key(lo.xyz), key(hi.xyz)
    uint32_t *voff, *foff;                           // [V], [F] kept rows before this one inside its block of CLEAN_WG
    uint32_t *vblk, *fblk;                           // [blocks] totals, then (clean_sums_kernel) kept rows before the block
    uint32_t* misc;                                  // [CLEAN_MISC_WORDS] the mesh's box, components, components kept, invalid faces
    int64_t vblocks, fblocks, bytes;
    __host__ CleanWs(void* base, int64_t V, int64_t F) {
        MeshCarver c(base);                                              // base == nullptr: only `bytes` is used
        vblocks = (V + CLEAN_WG - 1) / CLEAN_WG;
        fblocks = (F + CLEAN_WG - 1) / CLEAN_WG;
        misc = c.take<uint32_t>(CLEAN_MISC_WORDS);
        link = c.take<uint32_t>(V);
        parent = c.take<uint32_t>(V);
        lab = c.take<uint32_t>(V);
        ref = c.take<uint32_t>(V);
        cnt = c.take<uint32_t>(V);
        keep = c.take<uint32_t>(V);
        box = c.take<uint32_t>(6 * V);
        voff = c.take<uint32_t>(V);
        foff = c.take<uint32_t>(F);
        vblk = c.take<uint32_t>(vblocks);
        fblk = c.take<uint32_t>(fblocks);
        bytes = c.used();
    }
};

// The lanes among `pending` that hold the label of the first pending lane, as a mask; *leader is that lane.  Wave-uniform control flow.
__device__ __forceinline__ uint64_t clean_same_label(bool pending, uint32_t label, int lane, int* leader, uint32_t* leader_label) {
    const uint64_t pm = wave_ballot(pending);
    *leader = pm ? __ffsll((long long)pm) - 1 : 0;
    *leader_label = __shfl(label, *leader);
    return wave_ballot(pending && label == *leader_label);
}

__global__ __launch_bounds__(CLEAN_WG) void clean_init_kernel(uint32_t V, CleanWs ws) {
    const uint32_t v = blockIdx.x * CLEAN_WG + threadIdx.x;
    if (v >= V) return;
    ws.link[v] = v;
    ws.ref[v] = 0;
    ws.cnt[v] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) ws.box[6 * (size_t)v + k] = 0;
}

// link[x] = the smallest index x shares a face with (itself where there is none): a forest inside the components, written with
// atomicMin alone.  It loses edges -- the hook launch takes every edge again -- but leaves that launch little to unite.
__global__ __launch_bounds__(CLEAN_WG) void clean_link_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    const uint32_t f = blockIdx.x * CLEAN_WG + threadIdx.x, V = (uint32_t)a.V;
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    bool invalid = false;
    if (f < (uint32_t)a.F) {
        const int32_t* t = a.faces + 3 * (size_t)f;
        const int i = t[0], j = t[1], k = t[2];
        if (mesh_face_valid(i, j, k, V)) {
            ws.ref[i] = 1;                                                // the same value from every writer
            ws.ref[j] = 1;
            ws.ref[k] = 1;
            const uint32_t low = (uint32_t)min(i, min(j, k));
            if ((uint32_t)i != low) atomicMin(ws.link + i, low);
            if ((uint32_t)j != low) atomicMin(ws.link + j, low);
            if ((uint32_t)k != low) atomicMin(ws.link + k, low);
        } else {
            invalid = true;
        }
    }
    const uint64_t m = wave_ballot(invalid);
    if (m != 0 && lane == 0) atomicAdd(ws.misc + CLEAN_INVALID, (uint32_t)__popcll(m));
}

// parent[v] = the root of v in the link forest; nothing writes link[] in this launch, so plain loads.
__global__ __launch_bounds__(CLEAN_WG) void clean_compress_kernel(uint32_t V, CleanWs ws) {
    const uint32_t v = blockIdx.x * CLEAN_WG + threadIdx.x;
    if (v >= V) return;
    uint32_t x = v, p;
    while ((p = ws.link[x]) != x) x = p;
    ws.parent[v] = x;
}

__global__ __launch_bounds__(CLEAN_WG) void clean_hook_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    const uint32_t f = blockIdx.x * CLEAN_WG + threadIdx.x, V = (uint32_t)a.V;
    if (f >= (uint32_t)a.F) return;
    const int32_t* t = a.faces + 3 * (size_t)f;
    const int i = t[0], j = t[1], k = t[2];
    if (!mesh_face_valid(i, j, k, V)) return;
    // Start from the parents (members of the same sets).  Three equal parents: one set already, and no walk to the root, whose word
    // every walk of a large component ends on.
    const uint32_t pi = mesh_load(ws.parent + i), pj = mesh_load(ws.parent + j), pk = mesh_load(ws.parent + k);
    if (pi != pj || pi != pk) {
        const uint32_t r = pi != pj ? mesh_union(ws.parent, pi, pj) : pi;
        if (pk != r) mesh_union(ws.parent, r, pk);
    }
}

__global__ __launch_bounds__(CLEAN_WG) void clean_flatten_kernel(uint32_t V, CleanWs ws) {
    const uint32_t v = blockIdx.x * CLEAN_WG + threadIdx.x;
    if (v >= V) return;
    uint32_t x = v, p;
    while ((p = ws.parent[x]) != x) x = p;                                // nothing writes parent[] in this launch
    ws.lab[v] = x;
}

// cnt[label] += n through the workgroup's table in LDS (open addressing, a few probes); a label that finds no slot adds to memory itself.
__device__ __forceinline__ void clean_tally(uint32_t* keys, uint32_t* sums, uint32_t* cnt, uint32_t label, uint32_t n) {
    uint32_t slot = (label * 2654435761u) >> (32 - CLEAN_TALLY_BITS);
    for (int probe = 0; probe < 8; ++probe, slot = (slot + 1) & ((1u << CLEAN_TALLY_BITS) - 1)) {
        const uint32_t old = atomicCAS(keys + slot, CLEAN_NO_LABEL, label);
        if (old == CLEAN_NO_LABEL || old == label) {
            atomicAdd(sums + slot, n);
            return;
        }
    }
    atomicAdd(cnt + label, n);
}

// A workgroup takes 4 x CLEAN_FACE_CHUNKS consecutive chunks of 64 faces, a wave a chunk at a time.  The lanes that share the leading
// lane's label add their number together; every sum goes to the workgroup's table, which is added to memory once at the end: one
// atomicAdd per label and 4,096 faces, whichever way the components interleave in the face order.
__global__ __launch_bounds__(CLEAN_WG) void clean_faces_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    __shared__ uint32_t keys[1 << CLEAN_TALLY_BITS], sums[1 << CLEAN_TALLY_BITS];
    static_assert((1 << CLEAN_TALLY_BITS) == CLEAN_WG, "a slot per thread");
    const uint32_t V = (uint32_t)a.V, F = (uint32_t)a.F;
    const int lane = threadIdx.x & (DGS_WAVE - 1), wave = threadIdx.x >> 6;
    const uint32_t first = (blockIdx.x * (CLEAN_WG / DGS_WAVE) + wave) * (CLEAN_FACE_CHUNKS * DGS_WAVE);
    keys[threadIdx.x] = CLEAN_NO_LABEL;
    sums[threadIdx.x] = 0;
    __syncthreads();
    for (int chunk = 0; chunk < CLEAN_FACE_CHUNKS; ++chunk) {
        if (first + chunk * DGS_WAVE >= F) break;                         // the whole wave
        const uint32_t f = first + chunk * DGS_WAVE + lane;
        bool pending = false;
        uint32_t label = 0;
        if (f < F) {
            const int32_t* t = a.faces + 3 * (size_t)f;
            const int i = t[0];
            if (mesh_face_valid(i, t[1], t[2], V)) {
                pending = true;
                label = ws.lab[i];
            }
        }
#pragma unroll
        for (int round = 0; round < CLEAN_ROUNDS; ++round) {
            int leader;
            uint32_t leader_label;
            const uint64_t same = clean_same_label(pending, label, lane, &leader, &leader_label);
            if (same != 0 && lane == leader) clean_tally(keys, sums, ws.cnt, leader_label, (uint32_t)__popcll(same));
            pending = pending && !((same >> lane) & 1);
        }
        if (pending) clean_tally(keys, sums, ws.cnt, label, 1u);
    }
    __syncthreads();
    if (keys[threadIdx.x] != CLEAN_NO_LABEL) atomicAdd(ws.cnt + keys[threadIdx.x], sums[threadIdx.x]);
}

__global__ __launch_bounds__(CLEAN_WG) void clean_box_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    __shared__ uint32_t part[CLEAN_WG / DGS_WAVE][6];
    const uint32_t v = blockIdx.x * CLEAN_WG + threadIdx.x;
    const int lane = threadIdx.x & (DGS_WAVE - 1), wave = threadIdx.x >> 6;
    const bool have = v < (uint32_t)a.V && ws.ref[v] != 0;
    bool pending = have;
    uint32_t label = 0, key[6] = {0, 0, 0, 0, 0, 0};                       // 0: the identity of the maximum
    if (have) {
        label = ws.lab[v];
        const float* p = a.vertices + 3 * (size_t)v;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t k = mesh_float_key(p[c]);
            key[c] = ~k;
            key[3 + c] = k;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {                                         // the mesh's box: wave, workgroup, six atomics a workgroup
        const uint32_t m = mesh_wave_max(key[c]);
        if (lane == 0) part[wave][c] = m;
    }
#pragma unroll
    for (int round = 0; round < CLEAN_ROUNDS; ++round) {
        int leader;
        uint32_t leader_label;
        const uint64_t same = clean_same_label(pending, label, lane, &leader, &leader_label);
        const bool mine = (same >> lane) & 1;
        if (same != 0) {                                                  // wave-uniform
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const uint32_t m = mesh_wave_max(mine ? key[c] : 0u);
                if (lane == leader) mesh_raise(ws.box + 6 * (size_t)leader_label + c, m);
            }
        }
        pending = pending && !mine;
    }
    if (pending) {
#pragma unroll
        for (int c = 0; c < 6; ++c) mesh_raise(ws.box + 6 * (size_t)label + c, key[c]);
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        uint32_t m = 0;
#pragma unroll
        for (int w = 0; w < CLEAN_WG / DGS_WAVE; ++w) m = part[w][threadIdx.x] > m ? part[w][threadIdx.x] : m;
        if (m != 0) mesh_raise(ws.misc + CLEAN_BOX + threadIdx.x, m);
    }
}

// (dx * dx + dy * dy) + dz * dz of a box stored as {~key(lo), key(hi)}; fp64, STRICT_FP keeps the products and sums apart.
__device__ __forceinline__ double clean_diag2(const uint32_t* box) {
    double d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (double)mesh_float_unkey(box[3 + c]) - (double)mesh_float_unkey(~box[c]);
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
}

// threshold = pp * D2, pp = (p * p) of the header with p = min_diag_pct / 100.0 (two fp64 operations of the host).  One wave, lane c < 3
// squares the mesh box's extent along axis c: every fp64 operand comes from a per-lane load.  (With the six words loaded by one
// uniform address they sit in scalar registers, and hipcc of ROCm 7.2 crashes now and then while selecting v_cvt_f64_f32 for them.)
__global__ __launch_bounds__(DGS_WAVE) void clean_threshold_kernel(CleanWs ws, double pp) {
    __shared__ double square[3];
    if (threadIdx.x < 3) {
        const double d = (double)mesh_float_unkey(ws.misc[CLEAN_BOX + 3 + threadIdx.x]) - (double)mesh_float_unkey(~ws.misc[CLEAN_BOX + threadIdx.x]);
        square[threadIdx.x] = d * d;
    }
    __syncthreads();
    if (threadIdx.x == 0) *reinterpret_cast<double*>(ws.misc + CLEAN_THRESHOLD) = pp * (square[0] + square[1] + square[2]);
}

__global__ __launch_bounds__(CLEAN_WG) void clean_decide_kernel(DgsMeshCleanArgs a, CleanWs ws, int use_diag) {
    const uint32_t v = blockIdx.x * CLEAN_WG + threadIdx.x;
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    bool component = false, kept = false;
    if (v < (uint32_t)a.V) {
        const uint32_t n = ws.cnt[v];
        component = ws.lab[v] == v && n > 0;
        if (component) {
            bool removed = a.min_faces > 0 && n < (uint32_t)a.min_faces;
            if (use_diag) removed = removed || clean_diag2(ws.box + 6 * (size_t)v) < *reinterpret_cast<const double*>(ws.misc + CLEAN_THRESHOLD);
            kept = !removed;
        }
        ws.keep[v] = kept ? 1u : 0u;
    }
    const uint64_t mc = wave_ballot(component), mk = wave_ballot(kept);
    if (lane == 0 && mc != 0) atomicAdd(ws.misc + CLEAN_COMPONENTS, (uint32_t)__popcll(mc));
    if (lane == 0 && mk != 0) atomicAdd(ws.misc + CLEAN_KEPT, (uint32_t)__popcll(mk));
}

__device__ __forceinline__ bool clean_vertex_kept(const CleanWs& ws, uint32_t v) { return ws.ref[v] != 0 && ws.keep[ws.lab[v]] != 0; }

__device__ __forceinline__ bool clean_face_kept(const DgsMeshCleanArgs& a, const CleanWs& ws, uint32_t f, int (&t)[3]) {
    const int32_t* p = a.faces + 3 * (size_t)f;
    t[0] = p[0];
    t[1] = p[1];
    t[2] = p[2];
    return mesh_face_valid(t[0], t[1], t[2], (uint32_t)a.V) && ws.keep[ws.lab[t[0]]] != 0;
}

__global__ __launch_bounds__(CLEAN_WG) void clean_vscan_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    __shared__ uint32_t scratch[CLEAN_WG / DGS_WAVE + 1];
    const uint32_t v = blockIdx.x * CLEAN_WG + threadIdx.x;
    const bool in = v < (uint32_t)a.V;
    uint32_t total;
    const uint32_t before = block_exclusive_scan<CLEAN_WG>(in && clean_vertex_kept(ws, v) ? 1u : 0u, scratch, &total);
    if (in) ws.voff[v] = before;
    if (threadIdx.x == 0) ws.vblk[blockIdx.x] = total;
}

__global__ __launch_bounds__(CLEAN_WG) void clean_fscan_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    __shared__ uint32_t scratch[CLEAN_WG / DGS_WAVE + 1];
    const uint32_t f = blockIdx.x * CLEAN_WG + threadIdx.x;
    const bool in = f < (uint32_t)a.F;
    int t[3];
    uint32_t total;
    const uint32_t before = block_exclusive_scan<CLEAN_WG>(in && clean_face_kept(a, ws, f, t) ? 1u : 0u, scratch, &total);
    if (in) ws.foff[f] = before;
    if (threadIdx.x == 0) ws.fblk[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void clean_sums_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    __shared__ uint32_t scratch[1024 / DGS_WAVE + 1];
    const uint32_t nv = mesh_scan_blocks(ws.vblk, ws.vblocks, scratch);
    const uint32_t nf = mesh_scan_blocks(ws.fblk, ws.fblocks, scratch);
    if (threadIdx.x == 0) {
        a.counts[0] = nv;
        a.counts[1] = nf;
        a.counts[2] = ws.misc[CLEAN_COMPONENTS];
        a.counts[3] = ws.misc[CLEAN_KEPT];
        a.counts[4] = ws.misc[CLEAN_INVALID];
    }
}

// V = 0 or F = 0: nothing stays; with no vertices every face is invalid.
__global__ void clean_nothing_kernel(uint32_t* counts, uint32_t invalid) {
    if (threadIdx.x < 5) counts[threadIdx.x] = threadIdx.x == 4 ? invalid : 0u;
}

__global__ __launch_bounds__(CLEAN_WG) void clean_emit_vertices_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    const uint32_t v = blockIdx.x * CLEAN_WG + threadIdx.x;
    if (v >= (uint32_t)a.V || !clean_vertex_kept(ws, v)) return;
    const uint32_t at = ws.vblk[blockIdx.x] + ws.voff[v];
    if ((int64_t)at >= a.max_vertices) return;
    mesh_copy_vertex_bytes(a.vertices, v, a.out_vertices, at);
}

__global__ __launch_bounds__(CLEAN_WG) void clean_emit_faces_kernel(DgsMeshCleanArgs a, CleanWs ws) {
    const uint32_t f = blockIdx.x * CLEAN_WG + threadIdx.x;
    if (f >= (uint32_t)a.F) return;
    int t[3];
    const bool kept = clean_face_kept(a, ws, f, t);
    if (a.labels) a.labels[f] = mesh_face_valid(t[0], t[1], t[2], (uint32_t)a.V) ? (int32_t)ws.lab[t[0]] : -1;
    if (!kept) return;
    const uint32_t at = ws.fblk[blockIdx.x] + ws.foff[f];
    if ((int64_t)at >= a.max_faces) return;
    int32_t* out = a.out_faces + 3 * (size_t)at;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (int32_t)(ws.vblk[(uint32_t)t[c] / CLEAN_WG] + ws.voff[t[c]]);
}

static bool clean_args_ok(const DgsMeshCleanArgs* a) {
    return a && a->V >= 0 && a->F >= 0 && a->V <= CLEAN_MAX_ROWS && a->F <= CLEAN_MAX_ROWS && a->min_faces >= 0 && a->min_diag_pct >= 0 /* false for NaN */ &&
           (a->V == 0 || a->vertices) && (a->F == 0 || a->faces) && a->workspace && ((uintptr_t)a->workspace & 15) == 0 &&
           a->workspace_bytes >= CleanWs(nullptr, a->V, a->F).bytes;
}

}  // namespace dgs

extern "C" int64_t dgs_mesh_clean_workspace_bytes(int64_t V, int64_t F) {
    if (V < 0 || F < 0 || V > dgs::CLEAN_MAX_ROWS || F > dgs::CLEAN_MAX_ROWS) return 0;
    return dgs::CleanWs(nullptr, V, F).bytes;
}

extern "C" int dgs_mesh_clean_count(const DgsMeshCleanArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!clean_args_ok(a) || !a->counts) return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->V == 0 || a->F == 0) {
        hipLaunchKernelGGL(clean_nothing_kernel, dim3(1), dim3(DGS_WAVE), 0, st, a->counts, (uint32_t)(a->V == 0 ? a->F : 0));
        return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
    }
    const CleanWs ws(a->workspace, a->V, a->F);
    const dim3 wg(CLEAN_WG), vgrid((unsigned)ws.vblocks), fgrid((unsigned)ws.fblocks);
    if (hipMemsetAsync(ws.misc, 0, 4 * CLEAN_MISC_WORDS, st) != hipSuccess) return DGS_ERR_DEVICE;
    hipLaunchKernelGGL(clean_init_kernel, vgrid, wg, 0, st, (uint32_t)a->V, ws);
    hipLaunchKernelGGL(clean_link_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(clean_compress_kernel, vgrid, wg, 0, st, (uint32_t)a->V, ws);
    hipLaunchKernelGGL(clean_hook_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(clean_flatten_kernel, vgrid, wg, 0, st, (uint32_t)a->V, ws);
    const int64_t faces_per_wg = (int64_t)CLEAN_WG * CLEAN_FACE_CHUNKS;
    hipLaunchKernelGGL(clean_faces_kernel, dim3((unsigned)((a->F + faces_per_wg - 1) / faces_per_wg)), wg, 0, st, *a, ws);
    hipLaunchKernelGGL(clean_box_kernel, vgrid, wg, 0, st, *a, ws);
    const double p = a->min_diag_pct / 100.0;
    if (a->min_diag_pct > 0) hipLaunchKernelGGL(clean_threshold_kernel, dim3(1), dim3(DGS_WAVE), 0, st, ws, p * p);
    hipLaunchKernelGGL(clean_decide_kernel, vgrid, wg, 0, st, *a, ws, a->min_diag_pct > 0 ? 1 : 0);
    hipLaunchKernelGGL(clean_vscan_kernel, vgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(clean_fscan_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(clean_sums_kernel, dim3(1), dim3(1024), 0, st, *a, ws);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

extern "C" int dgs_mesh_clean_emit(const DgsMeshCleanArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!clean_args_ok(a) || a->max_vertices < 0 || a->max_faces < 0 || (a->max_vertices > 0 && !a->out_vertices) || (a->max_faces > 0 && !a->out_faces))
        return DGS_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->V == 0 || a->F == 0) {                                         // nothing stays; every face (if any) is invalid
        if (a->labels && a->F > 0 && hipMemsetAsync(a->labels, 0xff, 4 * (size_t)a->F, st) != hipSuccess) return DGS_ERR_DEVICE;
        return DGS_OK;
    }
    const CleanWs ws(a->workspace, a->V, a->F);
    if (a->max_vertices > 0) hipLaunchKernelGGL(clean_emit_vertices_kernel, dim3((unsigned)ws.vblocks), dim3(CLEAN_WG), 0, st, *a, ws);
    if (a->max_faces > 0 || a->labels) hipLaunchKernelGGL(clean_emit_faces_kernel, dim3((unsigned)ws.fblocks), dim3(CLEAN_WG), 0, st, *a, ws);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
