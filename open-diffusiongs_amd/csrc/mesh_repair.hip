// mesh_repair.hip -- repair of a triangle mesh on the device (include/dgs_mesh_repair.h DgsMeshRepairArgs; the order-free counterpart of
// the four repair filters of the reference's clean_mesh: meshing_remove_null_faces, meshing_remove_duplicate_faces,
// meshing_repair_non_manifold_edges(method=0), meshing_repair_non_manifold_vertices(vertdispratio=0), and the
// remove_unreferenced_vertices behind each), and the census of a mesh's topology.  The header holds the definition; this file is its
// kernel sequence.  The census (CENSUS = true) runs the same kernels without the areas, the duplicates and the marking.
//
// dgs_mesh_repair_count / dgs_mesh_topology (two memsets: the zeroed arrays, and the two tables' keys and the per-vertex minima to 0xff):
//   rep_face_kernel       thread = face: validity, area2 in fp64 (rep_area2), the null rule; invalid and null faces counted (one atomic
//                         a wave, issued only by a wave that has some).  fst[f] = the bits of (float)area2, the upper half of the
//                         face's key, or REP_DEAD.  A face that stays goes into the duplicate table: mesh_decimate.hip's table on vertex
//                         triples (atomicCAS of the face index into an empty slot, atomicMin into a slot of the same sorted triple,
//                         any other occupant: the next slot).  parent[3 f + k] = 3 f + k.
//   rep_edge_insert_kernel  thread = face, the next launch: a face whose slot holds another index is a duplicate (fst = REP_DUP).  A
//                         live face claims the slot of each of its three edges in the edge table (64-bit atomicCAS of a << 32 | b into
//                         an empty slot; a slot of the same key is the edge's; any other: the next slot), remembers it in eslot[],
//                         adds 1 to the slot's incidence and takes atomicMax(best, K_f).  A vertex of high valence spreads its faces
//                         over as many slots as it has edges: only the faces of ONE edge meet on a slot, two on a manifold edge.
//   rep_edge_second_kernel  thread = face: atomicMax(second, K_f) on each edge whose best is another face's.
//   rep_edge_mark_kernel  thread = face: on an edge of incidence >= 3 a face whose key is neither best nor second is marked (fst =
//                         REP_MARKED, its own word).  The face that is an edge's best counts the edge: non-manifold, and for the census
//                         border and manifold, summed over the wave and the workgroup in LDS, at most three atomics a workgroup.
//   rep_fan_kernel        thread = face: the surviving best face of an edge whose second face survives too (the census: an edge of
//                         incidence exactly 2) unites its corner at a with the other face's corner at a, and the same at b, in a
//                         lock-free union-find over the corner ids (csrc/mesh_common.h, mesh_union: nothing waits, and every access to
//                         parent[] in this launch is an agent-scope atomic).
//   rep_flatten_kernel    thread = corner, the next launch (plain loads see the final links): lab[c] = the root of c = its fan's label.
//                         A root takes atomicMin(vmin[vertex], c): one atomic a FAN, not one a corner -- the closed fan of 16,385 faces
//                         on one vertex is one atomic on that vertex's word, 300 tetrahedra on one vertex are 300.
//   rep_cscan_kernel      thread = corner: secondary = a root that is not its vertex's minimum: nm[vertex] = 1 (the same value from every
//                         writer), exclusive scan of the flags over the workgroup, block totals aside.
//   rep_vscan_kernel      thread = vertex: referenced = vmin set; scan, block totals aside, the non-manifold vertices in the upper half.
//   rep_fscan_kernel      thread = face: surviving; scan; duplicates and marked faces ride in the same word, ten bits each.
//   rep_sums_kernel       one workgroup: exclusive scans of the three lists of block totals (a piece of each list a thread, however many
//                         blocks there are), the other totals added up, the counts to the caller.
// dgs_mesh_repair_emit:
//   rep_emit_vertices_kernel  thread = vertex: a referenced vertex's 12 bytes to block base + offset.
//   rep_emit_faces_kernel     thread = face: a surviving face to block base + offset, each corner rewritten to its vertex's row (the
//                         primary fan) or to V_ref + the secondary root's rank; the corner that IS a secondary root writes the copy.
// The only atomics are integer: the tables' compare-and-swap / minimum / maximum / add, the union-find, the minima.  None of their final
// results depends on the order of arrival, and positions come from the scans: same input, same bytes.  STRICT_FP (dgs_amd/build.py): no
// fused multiply-add, so numpy (tests/mesh_repair_util.py) and the emulator build compute every area2 as the device does.
//
// Workspace: 60 B a face, 12 B a vertex, 4 B a slot of the duplicate table (2 F to 4 F slots), 28 B a slot of the edge table (6 F to
// 12 F slots).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dgs_device.h"
#include "dgs_mesh_repair.h"
#include "mesh_common.h"

namespace dgs {

typedef unsigned long long rep_u64;

constexpr int REP_WG = 256;
constexpr int64_t REP_MAX_V = (int64_t)1 << 30;
constexpr int64_t REP_MAX_F = (int64_t)1 << 28;      // 3 F corner ids and 12 F slots stay below 2^32
constexpr uint32_t REP_NONE = 0xffffffffu;           // no slot, no corner, no face
constexpr rep_u64 REP_NO_KEY = ~0ull;                // an empty slot of the edge table: a < 2^30 in every key
constexpr uint32_t REP_LIVE_MAX = 0x7f800000u;       // fst[f] <= the bits of +infinity: the face takes part; above: why it does not
constexpr uint32_t REP_DEAD = 0xffffffffu, REP_DUP = 0xfffffffeu, REP_MARKED = 0xfffffffdu;
enum { REP_INVALID = 0, REP_NULL = 1, REP_ERROR = 2, REP_BORDER = 3, REP_MANIFOLD = 4, REP_NONMANIFOLD = 5, REP_VREF = 6, REP_MISC_WORDS = 16 };

struct RepWs {
    uint32_t* misc;                                  // [REP_MISC_WORDS]
    uint32_t* ecount;                                // [eslots] the edge's incidence
    rep_u64 *ebest, *esecond;                        // [eslots] the two largest keys on the edge; 0: none
    uint32_t* nm;                                    // [V] 1: the vertex has a secondary fan
    rep_u64* ekey;                                   // [eslots] a << 32 | b, REP_NO_KEY = empty
    uint32_t* dtable;                                // [dslots] face indices, REP_NONE = empty
    uint32_t* vmin;                                  // [V] the smallest fan label of the vertex, REP_NONE = unreferenced
    uint32_t *fst, *fslot, *foff;                    // [F] key bits or the reason; slot in dtable; surviving faces before it in its block
    uint32_t *eslot, *parent, *lab, *coff;           // [3 F] by corner: the edge's slot (edge k: corners k, k + 1); union-find; label; scan
    uint32_t* voff;                                  // [V] referenced vertices before it in its block
    uint32_t *vblk, *vnm;                            // [vblocks] totals (then scanned); non-manifold vertices of the block
    uint32_t *fblk, *fdup, *fmark;                   // [fblocks] totals (then scanned); duplicates; marked faces
    uint32_t* cblk;                                  // [cblocks] totals (then scanned)
    int64_t eslots, dslots, vblocks, fblocks, cblocks, zero_bytes, ones_bytes, bytes;
    __host__ RepWs(void* base, int64_t V, int64_t F) {
        MeshCarver c(base);                                              // base == nullptr: only the sizes are used
        dslots = 64;
        while (dslots < 2 * F) dslots *= 2;
        eslots = 64;
        while (eslots < 6 * F) eslots *= 2;
        vblocks = (V + REP_WG - 1) / REP_WG;
        fblocks = (F + REP_WG - 1) / REP_WG;
        cblocks = (3 * F + REP_WG - 1) / REP_WG;
        misc = c.take<uint32_t>(REP_MISC_WORDS);                         // misc ... nm: zeroed by one memset
        ecount = c.take<uint32_t>(eslots);
        ebest = c.take<rep_u64>(eslots);
        esecond = c.take<rep_u64>(eslots);
        nm = c.take<uint32_t>(V);
        zero_bytes = c.used();
        ekey = c.take<rep_u64>(eslots);                                  // ekey ... vmin: set to 0xff by one memset
        dtable = c.take<uint32_t>(dslots);
        vmin = c.take<uint32_t>(V);
        ones_bytes = c.used() - zero_bytes;
        fst = c.take<uint32_t>(F);
        fslot = c.take<uint32_t>(F);
        foff = c.take<uint32_t>(F);
        eslot = c.take<uint32_t>(3 * F);
        parent = c.take<uint32_t>(3 * F);
        lab = c.take<uint32_t>(3 * F);
        coff = c.take<uint32_t>(3 * F);
        voff = c.take<uint32_t>(V);
        vblk = c.take<uint32_t>(vblocks);
        vnm = c.take<uint32_t>(vblocks);
        fblk = c.take<uint32_t>(fblocks);
        fdup = c.take<uint32_t>(fblocks);
        fmark = c.take<uint32_t>(fblocks);
        cblk = c.take<uint32_t>(cblocks);
        bytes = c.used();
    }
};

// The header's area2, five roundings a component of the normal and five more: every operand converted from a per-lane load.
__device__ __forceinline__ double rep_area2(const float* vertices, int i, int j, int k) {
    const float *pa = vertices + 3 * (size_t)i, *pb = vertices + 3 * (size_t)j, *pc = vertices + 3 * (size_t)k;
    const double ax = (double)pa[0], ay = (double)pa[1], az = (double)pa[2];
    const double ux = (double)pb[0] - ax, uy = (double)pb[1] - ay, uz = (double)pb[2] - az;
    const double wx = (double)pc[0] - ax, wy = (double)pc[1] - ay, wz = (double)pc[2] - az;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    return (nx * nx + ny * ny) + nz * nz;
}

// The slot of face f (valid, three distinct indices) in the duplicate table, REP_NONE when the probe found none.  The slots a triple
// passes are taken for good, so all faces of one triple end in one slot, which finally holds their smallest index.
__device__ __forceinline__ uint32_t rep_dup_slot(const int32_t* faces, const RepWs& ws, uint32_t f, int i, int j, int k) {
    const MeshTriple key = mesh_sorted((uint32_t)i, (uint32_t)j, (uint32_t)k);
    const uint32_t mask = (uint32_t)(ws.dslots - 1);
    uint32_t h = (key.s0 * 0x9E3779B1u) ^ (key.s1 * 0x85EBCA77u) ^ (key.s2 * 0xC2B2AE3Du);
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    for (int64_t probe = 0; probe < ws.dslots; ++probe) {
        const uint32_t slot = (h + (uint32_t)probe) & mask;
        const uint32_t old = atomicCAS(ws.dtable + slot, REP_NONE, f);
        if (old == REP_NONE) return slot;
        const int32_t* o = faces + 3 * (size_t)old;                       // a face that was inserted: valid, three distinct indices
        const MeshTriple theirs = mesh_sorted((uint32_t)o[0], (uint32_t)o[1], (uint32_t)o[2]);
        if (theirs.s0 == key.s0 && theirs.s1 == key.s1 && theirs.s2 == key.s2) {
            if (f < old) atomicMin(ws.dtable + slot, f);
            return slot;
        }
    }
    return REP_NONE;
}

// The slot of the edge {a, b} in the edge table, claimed if nobody has; REP_NONE when the probe found none.
__device__ __forceinline__ uint32_t rep_edge_slot(const RepWs& ws, uint32_t a, uint32_t b) {
    const rep_u64 key = a < b ? ((rep_u64)a << 32 | b) : ((rep_u64)b << 32 | a);
    const uint32_t mask = (uint32_t)(ws.eslots - 1);
    rep_u64 x = key;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    const uint32_t h = (uint32_t)x;
    for (int64_t probe = 0; probe < ws.eslots; ++probe) {
        const uint32_t slot = (h + (uint32_t)probe) & mask;
        const rep_u64 old = atomicCAS(ws.ekey + slot, REP_NO_KEY, key);
        if (old == REP_NO_KEY || old == key) return slot;
    }
    return REP_NONE;
}

__device__ __forceinline__ rep_u64 rep_key(uint32_t bits, uint32_t f) { return (rep_u64)bits << 32 | (rep_u64)(0xffffffffu - f); }
__device__ __forceinline__ uint32_t rep_key_face(rep_u64 key) { return 0xffffffffu - (uint32_t)key; }

template <bool CENSUS>
__global__ __launch_bounds__(REP_WG) void rep_face_kernel(DgsMeshRepairArgs a, RepWs ws) {
    const uint32_t f = blockIdx.x * REP_WG + threadIdx.x, V = (uint32_t)a.V;
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    bool invalid = false, null = false;
    if (f < (uint32_t)a.F) {
        const int32_t* t = a.faces + 3 * (size_t)f;
        const int i = t[0], j = t[1], k = t[2];
        uint32_t st = REP_DEAD, slot = REP_NONE;
        if (!mesh_face_valid(i, j, k, V)) {
            invalid = true;
        } else if (i == j || i == k || j == k) {
            null = true;
        } else if (CENSUS) {
            st = 0;                                                       // no areas: among the census's keys the smaller index wins
        } else {
            const double area2 = rep_area2(a.vertices, i, j, k);
            if (!(area2 > 0.0)) {
                null = true;
            } else {
                st = __float_as_uint((float)area2);
                slot = rep_dup_slot(a.faces, ws, f, i, j, k);
                if (slot == REP_NONE) {
                    ws.misc[REP_ERROR] = 1;
                    st = REP_DEAD;
                }
            }
        }
        ws.fst[f] = st;
        ws.fslot[f] = slot;
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) ws.parent[3 * f + c] = 3 * f + c;
    }
    const uint64_t mi = wave_ballot(invalid), mn = wave_ballot(null);
    if (mi != 0 && lane == 0) atomicAdd(ws.misc + REP_INVALID, (uint32_t)__popcll(mi));
    if (mn != 0 && lane == 0) atomicAdd(ws.misc + REP_NULL, (uint32_t)__popcll(mn));
}

template <bool CENSUS>
__global__ __launch_bounds__(REP_WG) void rep_edge_insert_kernel(DgsMeshRepairArgs a, RepWs ws) {
    const uint32_t f = blockIdx.x * REP_WG + threadIdx.x;
    if (f >= (uint32_t)a.F) return;
    const uint32_t st = ws.fst[f];
    if (st > REP_LIVE_MAX) return;
    if (!CENSUS && ws.dtable[ws.fslot[f]] != f) {                         // the table is final: written by the launch before
        ws.fst[f] = REP_DUP;
        return;
    }
    const int32_t* t = a.faces + 3 * (size_t)f;
    const uint32_t v[3] = {(uint32_t)t[0], (uint32_t)t[1], (uint32_t)t[2]};
    const rep_u64 key = rep_key(st, f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t slot = rep_edge_slot(ws, v[k], v[(k + 1) % 3]);
        ws.eslot[3 * f + k] = slot;
        if (slot == REP_NONE) {
            ws.misc[REP_ERROR] = 1;
            continue;
        }
        atomicAdd(ws.ecount + slot, 1u);
        atomicMax(ws.ebest + slot, key);
    }
}

__global__ __launch_bounds__(REP_WG) void rep_edge_second_kernel(DgsMeshRepairArgs a, RepWs ws) {
    const uint32_t f = blockIdx.x * REP_WG + threadIdx.x;
    if (f >= (uint32_t)a.F) return;
    const uint32_t st = ws.fst[f];
    if (st > REP_LIVE_MAX) return;
    const rep_u64 key = rep_key(st, f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t slot = ws.eslot[3 * f + k];
        if (slot != REP_NONE && ws.ebest[slot] != key) atomicMax(ws.esecond + slot, key);
    }
}

__device__ __forceinline__ uint32_t rep_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 1; d < DGS_WAVE; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

template <bool CENSUS>
__global__ __launch_bounds__(REP_WG) void rep_edge_mark_kernel(DgsMeshRepairArgs a, RepWs ws) {
    __shared__ uint32_t tally[3];
    const uint32_t f = blockIdx.x * REP_WG + threadIdx.x;
    const int lane = threadIdx.x & (DGS_WAVE - 1);
    if (threadIdx.x < 3) tally[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n[3] = {0, 0, 0};                                            // edges this face is the best of: border, manifold, non-manifold
    const uint32_t st = f < (uint32_t)a.F ? ws.fst[f] : REP_DEAD;
    if (st <= REP_LIVE_MAX) {
        const rep_u64 key = rep_key(st, f);
        bool marked = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t slot = ws.eslot[3 * f + k];
            if (slot == REP_NONE) continue;
            const uint32_t m = ws.ecount[slot];
            const rep_u64 best = ws.ebest[slot];
            if (best == key) {
                n[0] += m <= 1 ? 1u : 0u;
                n[1] += m == 2 ? 1u : 0u;
                n[2] += m >= 3 ? 1u : 0u;
            } else if (!CENSUS && m >= 3 && ws.esecond[slot] != key) {
                marked = true;
            }
        }
        if (marked) ws.fst[f] = REP_MARKED;
    }
#pragma unroll
    for (int c = CENSUS ? 0 : 2; c < 3; ++c) {
        const uint32_t s = rep_wave_sum(n[c]);
        if (s != 0 && lane == 0) atomicAdd(tally + c, s);
    }
    __syncthreads();
    if (threadIdx.x < 3 && tally[threadIdx.x] != 0) atomicAdd(ws.misc + REP_BORDER + threadIdx.x, tally[threadIdx.x]);
}

template <bool CENSUS>
__global__ __launch_bounds__(REP_WG) void rep_fan_kernel(DgsMeshRepairArgs a, RepWs ws) {
    const uint32_t f = blockIdx.x * REP_WG + threadIdx.x;
    if (f >= (uint32_t)a.F) return;
    const uint32_t st = ws.fst[f];
    if (st > REP_LIVE_MAX) return;
    const int32_t* t = a.faces + 3 * (size_t)f;
    const int v[3] = {t[0], t[1], t[2]};
    const rep_u64 key = rep_key(st, f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t slot = ws.eslot[3 * f + k];
        if (slot == REP_NONE || ws.ebest[slot] != key) continue;          // the edge's best face unites, once an edge
        const uint32_t m = ws.ecount[slot];
        if (CENSUS ? m != 2 : m < 2) continue;
        const uint32_t g = rep_key_face(ws.esecond[slot]);                // m >= 2: there is a second face
        if (g >= (uint32_t)a.F || ws.fst[g] > REP_LIVE_MAX) continue;     // marked by another of its edges: this edge is a border now
        const int32_t* o = a.faces + 3 * (size_t)g;
        const int va = v[k], vb = v[(k + 1) % 3];
        const uint32_t ja = o[0] == va ? 0u : (o[1] == va ? 1u : 2u), jb = o[0] == vb ? 0u : (o[1] == vb ? 1u : 2u);
        mesh_union(ws.parent, 3 * f + (uint32_t)k, 3 * g + ja);
        mesh_union(ws.parent, 3 * f + (uint32_t)((k + 1) % 3), 3 * g + jb);
    }
}

__global__ __launch_bounds__(REP_WG) void rep_flatten_kernel(DgsMeshRepairArgs a, RepWs ws) {
    const uint32_t c = blockIdx.x * REP_WG + threadIdx.x;
    if (c >= 3 * (uint32_t)a.F || ws.fst[c / 3] > REP_LIVE_MAX) return;
    uint32_t x = c, p;
    while ((p = ws.parent[x]) != x) x = p;                                // nothing writes parent[] in this launch
    ws.lab[c] = x;
    if (x == c) atomicMin(ws.vmin + a.faces[c], c);                       // a fan's root: one atomic a fan
}

__device__ __forceinline__ bool rep_secondary(const DgsMeshRepairArgs& a, const RepWs& ws, uint32_t c, uint32_t* vertex) {
    if (c >= 3 * (uint32_t)a.F || ws.fst[c / 3] > REP_LIVE_MAX || ws.lab[c] != c) return false;
    *vertex = (uint32_t)a.faces[c];
    return ws.vmin[*vertex] != c;
}

__global__ __launch_bounds__(REP_WG) void rep_cscan_kernel(DgsMeshRepairArgs a, RepWs ws) {
    __shared__ uint32_t scratch[REP_WG / DGS_WAVE + 1];
    const uint32_t c = blockIdx.x * REP_WG + threadIdx.x;
    uint32_t v = 0, total;
    const bool sec = rep_secondary(a, ws, c, &v);
    if (sec) ws.nm[v] = 1;                                                // the same value from every writer
    const uint32_t before = block_exclusive_scan<REP_WG>(sec ? 1u : 0u, scratch, &total);
    if (c < 3 * (uint32_t)a.F) ws.coff[c] = before;
    if (threadIdx.x == 0) ws.cblk[blockIdx.x] = total;
}

__global__ __launch_bounds__(REP_WG) void rep_vscan_kernel(DgsMeshRepairArgs a, RepWs ws) {
    __shared__ uint32_t scratch[REP_WG / DGS_WAVE + 1];
    const uint32_t v = blockIdx.x * REP_WG + threadIdx.x;
    const bool in = v < (uint32_t)a.V;
    uint32_t total;                                                       // referenced in the low half, non-manifold in the high half: <= 256 each
    const uint32_t before = block_exclusive_scan<REP_WG>((in && ws.vmin[v] != REP_NONE ? 1u : 0u) | (in && ws.nm[v] != 0 ? 0x10000u : 0u), scratch, &total);
    if (in) ws.voff[v] = before & 0xffffu;
    if (threadIdx.x == 0) {
        ws.vblk[blockIdx.x] = total & 0xffffu;
        ws.vnm[blockIdx.x] = total >> 16;
    }
}

__global__ __launch_bounds__(REP_WG) void rep_fscan_kernel(DgsMeshRepairArgs a, RepWs ws) {
    __shared__ uint32_t scratch[REP_WG / DGS_WAVE + 1];
    const uint32_t f = blockIdx.x * REP_WG + threadIdx.x;
    const uint32_t st = f < (uint32_t)a.F ? ws.fst[f] : REP_DEAD;
    uint32_t total;                                                       // three fields of ten bits: <= 256 each
    const uint32_t before = block_exclusive_scan<REP_WG>((st <= REP_LIVE_MAX ? 1u : 0u) | (st == REP_DUP ? 1u << 10 : 0u) | (st == REP_MARKED ? 1u << 20 : 0u), scratch, &total);
    if (f < (uint32_t)a.F) ws.foff[f] = before & 0x3ffu;
    if (threadIdx.x == 0) {
        ws.fblk[blockIdx.x] = total & 0x3ffu;
        ws.fdup[blockIdx.x] = (total >> 10) & 0x3ffu;
        ws.fmark[blockIdx.x] = total >> 20;
    }
}

__device__ __forceinline__ uint32_t rep_sum_blocks(const uint32_t* blk, int64_t n, uint32_t* scratch) {
    uint32_t s = 0, total;
    for (int64_t c = threadIdx.x; c < n; c += 1024) s += blk[c];
    block_exclusive_scan<1024>(s, scratch, &total);
    return total;
}

template <bool CENSUS>
__global__ __launch_bounds__(1024) void rep_sums_kernel(DgsMeshRepairArgs a, RepWs ws) {
    __shared__ uint32_t scratch[1024 / DGS_WAVE + 1];
    if (ws.misc[REP_ERROR]) {                                             // the whole workgroup
        if (!CENSUS && threadIdx.x < DGS_MESH_REPAIR_COUNTS) a.counts[threadIdx.x] = REP_NONE;
        if (CENSUS && threadIdx.x < DGS_MESH_TOPOLOGY_COUNTS) a.topology[threadIdx.x] = -1;
        return;
    }
    const uint32_t nv = mesh_scan_blocks(ws.vblk, ws.vblocks, scratch);
    const uint32_t added = mesh_scan_blocks(ws.cblk, ws.cblocks, scratch);
    const uint32_t nf = mesh_scan_blocks(ws.fblk, ws.fblocks, scratch);
    const uint32_t vnm = rep_sum_blocks(ws.vnm, ws.vblocks, scratch);
    const uint32_t dup = rep_sum_blocks(ws.fdup, ws.fblocks, scratch);
    const uint32_t marked = rep_sum_blocks(ws.fmark, ws.fblocks, scratch);
    if (threadIdx.x != 0) return;
    ws.misc[REP_VREF] = nv;
    if (CENSUS) {
        const int64_t border = ws.misc[REP_BORDER], manifold = ws.misc[REP_MANIFOLD], non = ws.misc[REP_NONMANIFOLD];
        a.topology[0] = border;
        a.topology[1] = manifold;
        a.topology[2] = non;
        a.topology[3] = vnm;
        a.topology[4] = nv;
        a.topology[5] = nf;
        a.topology[6] = (int64_t)nv - (border + manifold + non) + (int64_t)nf;
    } else {
        a.counts[0] = nv + added;
        a.counts[1] = nf;
        a.counts[2] = ws.misc[REP_INVALID];
        a.counts[3] = ws.misc[REP_NULL];
        a.counts[4] = dup;
        a.counts[5] = ws.misc[REP_NONMANIFOLD];
        a.counts[6] = marked;
        a.counts[7] = vnm;
        a.counts[8] = added;
        a.counts[9] = (uint32_t)a.V - nv;
    }
}

// V = 0: every face is invalid.  F = 0: every vertex is unreferenced.  The census of either is all zeros.
__global__ void rep_nothing_kernel(uint32_t* counts, int64_t* topology, uint32_t invalid, uint32_t unreferenced) {
    if (counts && threadIdx.x < DGS_MESH_REPAIR_COUNTS) counts[threadIdx.x] = threadIdx.x == 2 ? invalid : threadIdx.x == 9 ? unreferenced : 0u;
    if (topology && threadIdx.x < DGS_MESH_TOPOLOGY_COUNTS) topology[threadIdx.x] = 0;
}

__global__ __launch_bounds__(REP_WG) void rep_emit_vertices_kernel(DgsMeshRepairArgs a, RepWs ws) {
    const uint32_t v = blockIdx.x * REP_WG + threadIdx.x;
    if (ws.misc[REP_ERROR] || v >= (uint32_t)a.V || ws.vmin[v] == REP_NONE) return;
    const uint32_t at = ws.vblk[blockIdx.x] + ws.voff[v];
    if ((int64_t)at < a.max_vertices) mesh_copy_vertex_bytes(a.vertices, v, a.out_vertices, at);
}

__global__ __launch_bounds__(REP_WG) void rep_emit_faces_kernel(DgsMeshRepairArgs a, RepWs ws) {
    const uint32_t f = blockIdx.x * REP_WG + threadIdx.x;
    if (ws.misc[REP_ERROR] || f >= (uint32_t)a.F || ws.fst[f] > REP_LIVE_MAX) return;
    const uint32_t at = ws.fblk[blockIdx.x] + ws.foff[f], vref = ws.misc[REP_VREF];
    const int32_t* t = a.faces + 3 * (size_t)f;
    uint32_t row[3];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        const uint32_t c = 3 * f + k, v = (uint32_t)t[k], r = ws.lab[c];
        if (ws.vmin[v] == r) {
            row[k] = ws.vblk[v / REP_WG] + ws.voff[v];
        } else {
            row[k] = vref + ws.cblk[r / REP_WG] + ws.coff[r];
            if (r == c && (int64_t)row[k] < a.max_vertices) mesh_copy_vertex_bytes(a.vertices, v, a.out_vertices, row[k]);   // the fan's root writes the fan's copy
        }
    }
    if ((int64_t)at >= a.max_faces) return;
    int32_t* out = a.out_faces + 3 * (size_t)at;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (int32_t)row[k];
}

static bool rep_overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && pn > 0 && qn > 0 && a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

static bool rep_args_ok(const DgsMeshRepairArgs* a, bool census) {
    return a && a->V >= 0 && a->F >= 0 && a->V <= REP_MAX_V && a->F <= REP_MAX_F && (census || a->V == 0 || a->vertices) && (a->F == 0 || a->faces) &&
           a->workspace && (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0 && a->workspace_bytes >= RepWs(nullptr, a->V, a->F).bytes;
}

template <bool CENSUS>
static int rep_analyse(const DgsMeshRepairArgs* a, hipStream_t st) {
    if (a->V == 0 || a->F == 0) {
        hipLaunchKernelGGL(rep_nothing_kernel, dim3(1), dim3(DGS_WAVE), 0, st, CENSUS ? nullptr : a->counts, CENSUS ? a->topology : nullptr,
                           (uint32_t)(a->V == 0 ? a->F : 0), (uint32_t)(a->V == 0 ? 0 : a->V));
        return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
    }
    const RepWs ws(a->workspace, a->V, a->F);
    const dim3 wg(REP_WG), vgrid((unsigned)ws.vblocks), fgrid((unsigned)ws.fblocks), cgrid((unsigned)ws.cblocks);
    if (hipMemsetAsync(ws.misc, 0, (size_t)ws.zero_bytes, st) != hipSuccess) return DGS_ERR_DEVICE;
    if (hipMemsetAsync(ws.ekey, 0xff, (size_t)ws.ones_bytes, st) != hipSuccess) return DGS_ERR_DEVICE;
    hipLaunchKernelGGL(rep_face_kernel<CENSUS>, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_edge_insert_kernel<CENSUS>, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_edge_second_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_edge_mark_kernel<CENSUS>, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_fan_kernel<CENSUS>, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_flatten_kernel, cgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_cscan_kernel, cgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_vscan_kernel, vgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_fscan_kernel, fgrid, wg, 0, st, *a, ws);
    hipLaunchKernelGGL(rep_sums_kernel<CENSUS>, dim3(1), dim3(1024), 0, st, *a, ws);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}

}  // namespace dgs

extern "C" int64_t dgs_mesh_repair_workspace_bytes(int64_t V, int64_t F) {
    if (V < 0 || F < 0 || V > dgs::REP_MAX_V || F > dgs::REP_MAX_F) return 0;
    return dgs::RepWs(nullptr, V, F).bytes;
}

extern "C" int dgs_mesh_repair_count(const DgsMeshRepairArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!rep_args_ok(a, false) || !a->counts) return DGS_ERR_INVALID_ARGUMENT;
    return rep_analyse<false>(a, static_cast<hipStream_t>(stream));
}

extern "C" int dgs_mesh_topology(const DgsMeshRepairArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!rep_args_ok(a, true) || !a->topology) return DGS_ERR_INVALID_ARGUMENT;
    return rep_analyse<true>(a, static_cast<hipStream_t>(stream));
}

extern "C" int dgs_mesh_repair_emit(const DgsMeshRepairArgs* a, dgs_stream_t stream) {
    using namespace dgs;
    if (!rep_args_ok(a, false) || a->max_vertices < 0 || a->max_faces < 0 || (a->max_vertices > 0 && !a->out_vertices) || (a->max_faces > 0 && !a->out_faces))
        return DGS_ERR_INVALID_ARGUMENT;
    const int64_t vb = 12 * a->max_vertices, fb = 12 * a->max_faces;
    const void* outs[2] = {a->out_vertices, a->out_faces};
    const int64_t sizes[2] = {vb, fb};
    for (int o = 0; o < 2; ++o) {
        if (rep_overlap(outs[o], sizes[o], a->vertices, 12 * a->V) || rep_overlap(outs[o], sizes[o], a->faces, 12 * a->F) ||
            rep_overlap(outs[o], sizes[o], a->workspace, a->workspace_bytes))
            return DGS_ERR_INVALID_ARGUMENT;
    }
    if (rep_overlap(a->out_vertices, vb, a->out_faces, fb)) return DGS_ERR_INVALID_ARGUMENT;
    if (a->V == 0 || a->F == 0) return DGS_OK;                           // nothing stays
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RepWs ws(a->workspace, a->V, a->F);
    if (a->max_vertices > 0) hipLaunchKernelGGL(rep_emit_vertices_kernel, dim3((unsigned)ws.vblocks), dim3(REP_WG), 0, st, *a, ws);
    if (a->max_vertices > 0 || a->max_faces > 0) hipLaunchKernelGGL(rep_emit_faces_kernel, dim3((unsigned)ws.fblocks), dim3(REP_WG), 0, st, *a, ws);
    return hipGetLastError() == hipSuccess ? DGS_OK : DGS_ERR_DEVICE;
}
