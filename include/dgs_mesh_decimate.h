/* dgs_mesh_decimate.h -- C ABI of the mesh decimation on the device (csrc/mesh_decimate.hip): vertex clustering on a uniform grid of
 * n cells per axis, with the faces that collapse or coincide removed.
 *
 * The reference ends GaussianModel.extract_mesh with decimate_mesh(vertices, triangles, decimate_target) (pymeshlab's quadric edge
 * collapse, a sequential priority-queue algorithm whose result depends on the order of its operations) and carries MeshLab's other
 * decimation filter, meshing_decimation_clustering, as the commented alternative.  Clustering has an order-free definition, stated
 * here; the mesh stays on the device and five integers come back to the host.  Clustering can leave non-manifold edges where a thin
 * part of the mesh collapses.
 *
 * Definition (order-free, so the result can be pinned bit for bit).  Inputs: vertices f32 [V, 3], faces i32 [F, 3], n in [1, 1024].
 *   valid       A face is VALID iff its three indices lie in [0, V).  An invalid face is never dereferenced; it is dropped and counted.
 *   referenced  A vertex is REFERENCED iff a valid face names it.  Only referenced vertices take part in anything below.
 *   box         lo, hi fp32 [3]: the exact minima and maxima over the referenced vertices.  ext = max_k((double)hi_k - (double)lo_k).
 *               If there is no valid face, or ext == 0 (or ext is not a number), nothing is output: V' = F' = 0, and every valid
 *               face counts as degenerate.  Otherwise inv = (double)n / ext.
 *   cell        For a referenced vertex and axis k: u_k = ((double)x_k - (double)lo_k) * inv, c_k = min(n - 1, (int)floor(u_k)); the
 *               cell index is (c_x * n + c_y) * n + c_z.  Cells are cubes anchored at lo; the short axes use only some of them.
 *   offset      q_k = llrint((u_k - (double)c_k) * 1048576.0), round to nearest, ties to even: the vertex's place inside its cell in
 *               fixed point.  It lies in [0, 2^20], and it is 2^20 only for a coordinate equal to hi on the longest axis.
 *   cluster     the set of referenced vertices of one cell.  Per cluster: count, an integer, and sum_k, the 64-bit integer sum of
 *               q_k (at most 2^30 * 2^20 = 2^50, so it converts to fp64 exactly).
 *   position    p_k = (float)((double)lo_k + ((double)c_k + (double)sum_k / ((double)count * 1048576.0)) / inv): every fp64 operation
 *               rounded on its own (no fused multiply-add, no reassociation), the final conversion round to nearest even.
 *   faces       A valid face (a, b, c) maps to the cells (A, B, C) of its corners.  It is DEGENERATE iff two of them are equal;
 *               degenerate faces are dropped and counted.  Two non-degenerate faces are DUPLICATES iff {A, B, C} is the same
 *               unordered set (VCG's RemoveDuplicateFace rule, what meshing_remove_duplicate_faces of clean_mesh does); of a set of
 *               duplicates the face with the smallest input index stays, the others are dropped and counted.
 *   output      the kept faces in input order, their corner order unchanged (the orientation survives), their indices renumbered to
 *               the output vertices; the output vertices are the clusters a kept face refers to, in ascending cell index, with
 *               position p.  A cluster that only degenerate or duplicate faces touch is not output.
 *   counts      uint32 [5] = {V', F', degenerate faces, duplicate faces dropped, invalid faces}; they add up to F without V'.
 * Coordinates that are not finite give unspecified positions and decisions and never an access out of range: c_k is clamped into
 * [0, n - 1] and q_k into [0, 2^20] whatever the conversions yield.
 *
 * The definition is invariant under renaming: permuting the input vertices (faces renumbered to match) gives the same output vertex
 * bytes; permuting the faces gives the same vertex bytes and the same set of unordered faces.
 *
 * Two calls, because the caller allocates (the pattern of dgs_mesh_clean.h):
 *     dgs_mesh_decimate_count  fills the workspace and writes counts;
 *     -- the caller reads the five numbers (the one host synchronisation) and allocates --
 *     dgs_mesh_decimate_emit   with the SAME inputs and workspace: writes out_vertices [min(V', max_vertices)] and out_faces
 *                              [min(F', max_faces)]; nothing beyond them.  It may be repeated.
 * Device pointers, no allocation, no host synchronisation.  Occupied cells are marked in a mask of n^3 bits (atomic or); a cell's rank
 * among them is a prefix scan plus a population count; count and sum are integer atomic adds per cluster; the duplicate of the smallest
 * index is found in an open-addressing table of face indices (compare-and-swap into an empty slot, atomic minimum into a slot of the
 * same cells; a slot's cells never change once set).  Those are the only atomics: none of their final results depends on the order
 * in which they arrive, and every output position comes from a prefix scan, so the same input gives the same bytes in every run.
 * The table has more slots than faces, so a probe always ends; should one not, all five counts read 0xffffffff and emit writes nothing.
 *
 * Returns DGS_OK or a negative DgsStatus; DGS_ERR_INVALID_ARGUMENT when V or F is negative or above 2^30, n is outside [1, 1024], a
 * pointer the call uses is missing (`vertices` / `faces` may be NULL only when V / F is 0), max_vertices / max_faces < 0, or the
 * workspace is too small or not 16-byte aligned.  V = 0 or F = 0 is valid: nothing is output (with V = 0 every face is invalid), and
 * no kernel that indexes the inputs is launched. */
#ifndef DGS_MESH_DECIMATE_H
#define DGS_MESH_DECIMATE_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DgsMeshDecimateArgs {
    int64_t V, F;              /* rows of `vertices` and `faces`, each in [0, 2^30]                              */
    const float* vertices;     /* f32 [V, 3]                                                                     */
    const int32_t* faces;      /* i32 [F, 3]                                                                     */
    int32_t n;                 /* grid cells per axis, in [1, 1024]                                              */
    uint32_t* counts;          /* count: out uint32 [5] = {V', F', degenerate, duplicates dropped, invalid faces} */
    float* out_vertices;       /* emit: out f32 [max_vertices, 3]                                                */
    int32_t* out_faces;        /* emit: out i32 [max_faces, 3]                                                   */
    int64_t max_vertices;      /* emit: rows of `out_vertices` that may be written                               */
    int64_t max_faces;         /* emit: rows of `out_faces` that may be written                                  */
    void* workspace;           /* [dgs_mesh_decimate_workspace_bytes(V, F, n)], 16-byte aligned; count -> emit   */
    int64_t workspace_bytes;
} DgsMeshDecimateArgs;

int64_t dgs_mesh_decimate_workspace_bytes(int64_t V, int64_t F, int32_t n);   /* 0 for unsupported sizes; grows with n */
int dgs_mesh_decimate_count(const DgsMeshDecimateArgs* args, dgs_stream_t stream);
int dgs_mesh_decimate_emit(const DgsMeshDecimateArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
