/* dgs_mesh.h -- C ABI of marching cubes on the device (csrc/mesh.hip): the triangle mesh of the level set occ = level of the grid
 * dgs_gaussian_field (dgs_field.h) writes.
 *
 * Replaces `mcubes.marching_cubes(occ.cpu().numpy(), density_thresh)` of GaussianModel.extract_mesh,
 * diffusionGS/models/gsrenderer/gs_core.py:855-860: the grid stays on the device; two integers come back to the host.
 *
 *     sample (x, y, z) of occ [X, Y, Z] (z fastest) is INSIDE iff occ > level (equality and NaN are outside);
 *     cell (x, y, z), x < X - 1, y < Y - 1, z < Z - 1: corner k at (x + (k >> 2 & 1), y + (k >> 1 & 1), z + (k & 1)),
 *         case = sum of inside(corner k) << k, triangles of the case from csrc/mc_table.h (tools/make_mc_table.py is the table's
 *         specification; edge e = 4 * axis + r runs one step along +axis from the corner (0, r >> 1, r & 1) for axis 0,
 *         (r >> 1, 0, r & 1) for axis 1, (r >> 1, r & 1, 0) for axis 2).
 * The result is what one sequential loop would give, so it is reproducible bit for bit:
 *     vertices  f32 [V, 3] in index coordinates, one per crossed edge = pair of samples (s, s + e_axis) with different inside flags,
 *               ordered by the linear index (x * Y + y) * Z + z of s, then by axis 0, 1, 2.  With a = occ[s], b = occ[s + e_axis]:
 *               t = (level - a) / (b - a) in fp32 (two subtractions, one correctly rounded division), the coordinate along the axis
 *               is (float)index + t (one fp32 addition), the two others are the integer indices.
 *     triangles i32 [F, 3] of vertex indices, ordered by the cell's linear index (x * (Y - 1) + y) * (Z - 1) + z, then in the table's
 *               order; wound so that the normals point from inside to outside.  Every vertex is used by at least one triangle.
 *
 * Two calls, because the caller allocates:
 *     dgs_marching_cubes_count   fills the workspace and writes {V, F} to `counts` (device);
 *     -- the caller reads the two numbers (the one host synchronisation) and allocates --
 *     dgs_marching_cubes_emit    with the SAME occ, level and workspace: writes vertices [min(V, max_vertices)] and triangles
 *                                [min(F, max_triangles)], nothing beyond them.
 * Device pointers, no allocation, no host synchronisation, no atomics.  Returns DGS_OK or a negative DgsStatus;
 * DGS_ERR_INVALID_ARGUMENT when X, Y or Z < 2, X * Y * Z > 2^30 (3 * samples fits the uint32 counters), level is NaN, a pointer the
 * call uses is missing, max_vertices / max_triangles < 0 or the workspace is too small or not 16-byte aligned.  F is counted modulo
 * 2^32: a mesh of more than 4.29e9 triangles (51 GB of indices) is outside the contract; stores stay inside max_triangles even then. */
#ifndef DGS_MESH_H
#define DGS_MESH_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DgsMeshArgs {
    int32_t X, Y, Z;           /* samples per axis; the grid need not be cubic                                 */
    float level;               /* inside iff occ > level                                                       */
    const float* occ;          /* f32 [X, Y, Z], z fastest                                                     */
    uint32_t* counts;          /* count: out uint32 [2] = {V, F}                                               */
    float* vertices;           /* emit: out f32 [max_vertices, 3]                                              */
    int32_t* triangles;        /* emit: out i32 [max_triangles, 3]                                             */
    int64_t max_vertices;      /* emit: rows of `vertices` that may be written                                 */
    int64_t max_triangles;     /* emit: rows of `triangles` that may be written                                */
    void* workspace;           /* [dgs_marching_cubes_workspace_bytes(X, Y, Z)], 16-byte aligned; count -> emit */
    int64_t workspace_bytes;
} DgsMeshArgs;

int64_t dgs_marching_cubes_workspace_bytes(int32_t X, int32_t Y, int32_t Z);   /* 0 for an unsupported grid */
int dgs_marching_cubes_count(const DgsMeshArgs* args, dgs_stream_t stream);
int dgs_marching_cubes_emit(const DgsMeshArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
