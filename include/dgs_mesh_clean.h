/* dgs_mesh_clean.h -- C ABI of the mesh clean-up on the device (csrc/mesh_clean.hip): drop the small connected components of a
 * triangle mesh and the vertices nothing refers to any more.
 *
 * Replaces, for the mesh dgs_marching_cubes_emit (dgs_mesh.h) writes, the two filters of the reference's clean_mesh that remove the
 * "floaters" next to the object,
 *     meshing_remove_connected_component_by_diameter(mincomponentdiag = PercentageValue(min_d))     and
 *     meshing_remove_connected_component_by_face_number(mincomponentsize = min_f),
 * each followed by remove_unreferenced_vertices; the mesh stays on the device and five integers come back to the host.
 *
 * Definition (order-free, so the result can be pinned bit for bit).  Inputs: vertices f32 [V, 3], faces i32 [F, 3].
 *   valid      A face is VALID iff its three indices lie in [0, V).  An invalid face is never dereferenced, belongs to no component
 *              and is dropped.
 *   component  Two valid faces are in one component iff a chain of valid faces, each sharing a vertex INDEX with the next, connects
 *              them.  The component's canonical label is the smallest vertex index it contains.  On a closed manifold mesh (what
 *              marching cubes gives away from the grid's boundary) this is the partition of pymeshlab's face-face (edge) adjacency;
 *              two closed pieces that touch in a single vertex are ONE component here.
 *   n          the component's number of faces.
 *   lo, hi     fp32 [3]: the bounding box over the vertices the component's faces refer to (exact: minima and maxima of inputs).
 *   d2         dx * dx + dy * dy + dz * dz in fp64 with dx = (double)hi.x - (double)lo.x and likewise dy, dz; the products are summed
 *              in that order, ((dx * dx + dy * dy) + dz * dz), every operation rounded on its own (no fused multiply-add).
 *   D2         the same quantity of the box over ALL vertices that valid faces refer to.
 *   removal    A component is removed iff   min_faces > 0  and  n < min_faces
 *                                     or    min_diag_pct > 0  and  d2 < (p * p) * D2   with p = min_diag_pct / 100.0 (fp64).
 *              Both comparisons are strict, as VCG's are: a component of exactly min_faces faces stays, and so does a mesh that is
 *              one component at min_diag_pct = 100.  The reference applies the diameter filter first and the face-number filter to
 *              what is left; that composition equals this rule, because only the diameter test depends on the mesh's box and it runs
 *              first, on the whole mesh.
 *   output     the faces of the components that stay, in input order, their indices renumbered to the kept vertices; the kept
 *              vertices are those a kept face refers to, in input order, their 12 bytes copied unchanged (so vertices no face refers
 *              to are dropped too: remove_unreferenced_vertices).
 *   labels     optional, i32 [F]: the canonical label of each INPUT face, -1 for an invalid face.
 * Coordinates that are not finite give an unspecified keep / remove decision and never an access out of range.
 *
 * Two calls, because the caller allocates (the pattern of dgs_mesh.h):
 *     dgs_mesh_clean_count   fills the workspace and writes counts uint32 [5] = {V', F', components, components kept, invalid faces};
 *     -- the caller reads the five numbers (the one host synchronisation) and allocates --
 *     dgs_mesh_clean_emit    with the SAME inputs and workspace: writes out_vertices [min(V', max_vertices)], out_faces
 *                            [min(F', max_faces)] and, when `labels` is given, labels [F]; nothing beyond them.
 * Device pointers, no allocation, no host synchronisation.  The components are found with a union-find over the vertex indices whose
 * links only ever move to a smaller index (compare-and-swap); per component the face count is an integer atomic add and the box an
 * atomic minimum / maximum of the order-preserving uint32 image of the floats.  Those are the only atomics: none of their results
 * depends on the order in which they arrive, and every output position comes from a prefix scan, so the same input gives the same
 * bytes in every run.
 *
 * Returns DGS_OK or a negative DgsStatus; DGS_ERR_INVALID_ARGUMENT when V or F is negative or above 2^30, min_faces is negative,
 * min_diag_pct is NaN or negative, a pointer the call uses is missing (`vertices` / `faces` may be NULL only when V / F is 0),
 * max_vertices / max_faces < 0, or the workspace is too small or not 16-byte aligned.  V = 0 or F = 0 is valid: nothing stays (with
 * V = 0 every face is invalid), and no kernel that indexes the inputs is launched. */
#ifndef DGS_MESH_CLEAN_H
#define DGS_MESH_CLEAN_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DgsMeshCleanArgs {
    int64_t V, F;              /* rows of `vertices` and `faces`, each in [0, 2^30]                            */
    const float* vertices;     /* f32 [V, 3]                                                                   */
    const int32_t* faces;      /* i32 [F, 3]                                                                   */
    int32_t min_faces;         /* remove components of fewer faces; 0 = off                                    */
    double min_diag_pct;       /* remove components whose box diagonal is below this percentage of the mesh's; 0 = off */
    uint32_t* counts;          /* count: out uint32 [5] = {V', F', components, components kept, invalid faces}  */
    float* out_vertices;       /* emit: out f32 [max_vertices, 3]                                              */
    int32_t* out_faces;        /* emit: out i32 [max_faces, 3]                                                 */
    int32_t* labels;           /* emit: optional out i32 [F]                                                   */
    int64_t max_vertices;      /* emit: rows of `out_vertices` that may be written                             */
    int64_t max_faces;         /* emit: rows of `out_faces` that may be written                                */
    void* workspace;           /* [dgs_mesh_clean_workspace_bytes(V, F)], 16-byte aligned; count -> emit       */
    int64_t workspace_bytes;
} DgsMeshCleanArgs;

int64_t dgs_mesh_clean_workspace_bytes(int64_t V, int64_t F);   /* 0 for unsupported sizes */
int dgs_mesh_clean_count(const DgsMeshCleanArgs* args, dgs_stream_t stream);
int dgs_mesh_clean_emit(const DgsMeshCleanArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
