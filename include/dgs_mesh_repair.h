/* dgs_mesh_repair.h -- C ABI of the mesh repair on the device (csrc/mesh_repair.hip): null and duplicate faces removed, non-manifold
 * edges brought down to two faces, non-manifold vertices split into one vertex per fan, and a census of a mesh's topology.
 *
 * The reference's clean_mesh runs, with repair=True, pymeshlab's meshing_remove_duplicate_faces, meshing_remove_null_faces,
 * meshing_repair_non_manifold_edges(method=0) and meshing_repair_non_manifold_vertices(vertdispratio=0), each followed by
 * remove_unreferenced_vertices.  MeshLab's edge repair deletes the smallest faces of an edge one after another in mesh order; the
 * definition here is its order-free form, so the result can be pinned bit for bit.  The mesh stays on the device and ten integers come
 * back to the host.  Merging close vertices and isotropic remeshing are not part of this.
 *
 * Definition.  Inputs: vertices f32 [V, 3], faces i32 [F, 3].  Face index f; the corner k of face f has the CORNER ID 3 f + k.
 *   1 valid     A face is VALID iff its three indices lie in [0, V).  An invalid face is never dereferenced; it is dropped and counted.
 *     null      For a valid face (a, b, c), in its stored corner order, in fp64 from the fp32 coordinates:
 *                   u = (double)p_b - (double)p_a,  w = (double)p_c - (double)p_a                    (per axis)
 *                   n_x = u_y * w_z - u_z * w_y,  n_y = u_z * w_x - u_x * w_z,  n_z = u_x * w_y - u_y * w_x
 *                   area2 = (n_x * n_x + n_y * n_y) + n_z * n_z
 *               every operation rounded on its own (no fused multiply-add, no reassociation).  The face is NULL iff two of its indices
 *               are equal or !(area2 > 0): a zero area and an area that is not a number (what a NaN coordinate, or two infinite ones on
 *               one axis, give) land here.  An area2 of +infinity is above 0: such a face stays.  Null faces are dropped and counted.
 *   2 duplicate Of the valid, non-null faces that name the same set of three vertices, in any corner order and either orientation, the
 *               one of the smallest face index stays; the others are dropped and counted.  The faces now left are LIVE.
 *   3 edges     The undirected edge {a, b}, a < b, has the incidence m = the number of live faces that name both.  m = 1: a BORDER
 *               edge; m = 2: MANIFOLD; m >= 3: NON-MANIFOLD.  The rank key of a live face is
 *                   K_f = (uint64)bits((float)area2) << 32 | (0xFFFFFFFF - f)            (float): round to nearest even
 *               the larger area wins, then the smaller index; the float is not negative, so its bits order as it does.  On every
 *               non-manifold edge the two faces of the largest keys are kept by that edge and every other face on it is MARKED.  A face
 *               marked by any of its three edges is removed and counted.  One round: incidences only go down, so afterwards no edge has
 *               more than two faces.  An edge that kept a face which another edge removed is left with one face (or none): it becomes
 *               a border edge of the output, it is not repaired further.
 *   4 fans      Over the corners of the faces that SURVIVE step 3: two corners are joined iff they name the same vertex and their faces
 *               share an edge at that vertex (that edge then has exactly those two surviving faces).  The classes of the corners of a
 *               vertex are its FANS; the LABEL of a fan is its smallest corner id.  A vertex with two or more fans is NON-MANIFOLD: its
 *               fan of the smallest label is PRIMARY and keeps the vertex, every other fan gets a COPY of it: the same 12 bytes, no
 *               displacement (vertdispratio = 0).
 *   5 output    Vertices: first the input vertices that a surviving face names, in index order (the others are UNREFERENCED: dropped
 *               and counted); then the copies, in increasing order of their fans' labels.  Faces: the surviving faces in input order,
 *               corner order and orientation unchanged, every corner rewritten to the output row of its fan.  A manifold mesh without
 *               invalid, null or duplicate faces and without unreferenced vertices comes back byte for byte.
 *   6 counts    uint32 [10] = {V', F', invalid faces, null faces, duplicate faces dropped, non-manifold edges found, faces removed by
 *               step 3, non-manifold vertices found, vertices added (copies), unreferenced vertices dropped}.
 *               F' = F - invalid - null - duplicate - removed;  V' = V - unreferenced + added.
 *   7 census    dgs_mesh_topology, no output mesh and no coordinates: over the valid faces with three distinct indices (duplicates
 *               count as often as they occur; areas are not looked at) int64 [7] = {border edges, manifold edges, non-manifold edges,
 *               non-manifold vertices, referenced vertices, faces, Euler characteristic V_ref - E + F}, with the incidences of step 3
 *               over those faces and the fans of step 4 joined through the edges of incidence exactly 2.  It shares no decision with
 *               the repair beyond the tables it is built from, and reads a raw mesh as well as a repaired one.
 * Coordinates only enter area2, and through it the null rule and the keys: no address depends on a coordinate.
 *
 * Properties.  The same input gives the same bytes in every run.  Renaming the vertices (faces renumbered to match) gives the same mesh
 * as a set of coordinate triangles; the output rows may come in another order, because a copy's place follows its fan's label, a corner
 * id, and the kept duplicate and the keys do not depend on vertex names.  Permuting the faces can change the tie-breaks of steps 2 to 4
 * (which duplicate stays, which of two faces of equal area an edge keeps, which fan is primary).  Orientation is neither checked nor
 * repaired: two faces that run along an edge in the same direction are joined like any others.
 *
 * Two calls, because the caller allocates (the pattern of dgs_mesh_clean.h):
 *     dgs_mesh_repair_count  does all of the analysis in the workspace and writes counts;
 *     -- the caller reads the ten numbers (the one host synchronisation) and allocates --
 *     dgs_mesh_repair_emit   with the SAME inputs and workspace: writes out_vertices [min(V', max_vertices)] and out_faces
 *                            [min(F', max_faces)]; nothing beyond them.  It may be repeated.
 * dgs_mesh_topology is one call on a workspace of the same size.  Device pointers, no allocation, no host synchronisation.
 * Duplicates meet in an open-addressing table of face indices keyed by the sorted triple (compare-and-swap into an empty slot, atomic
 * minimum into a slot of the same triple); edges in an open-addressing table keyed by a << 32 | b with at least 6 F slots (64-bit
 * compare-and-swap), each slot with an incidence (atomic add) and the two largest keys (64-bit atomic maximum, one launch each); fans
 * in a lock-free union-find over the 3 F corner ids whose links only decrease, so a root is its class's smallest id.  Which slot an
 * edge lands in depends on the order of arrival; nothing that is output does, and every output position comes from a prefix scan.
 * Every probe is bounded by the table's capacity and no loop waits for another workgroup; should a probe find no slot (it cannot:
 * each table has at least twice as many slots as keys), all ten counts (all seven census numbers) read all-ones and emit writes nothing.
 *
 * Limits: V in [0, 2^30] (an edge key holds two 30-bit indices), F in [0, 2^28] (3 F corner ids and the slots of a table of 6 F to
 * 12 F entries are 32-bit numbers).  The workspace takes 60 B a face, 8 to 16 B a face for the duplicate table, 28 B a slot of the edge
 * table (168 to 336 B a face) and 12 B a vertex.
 *
 * Returns DGS_OK or a negative DgsStatus; DGS_ERR_INVALID_ARGUMENT when V or F is outside its limits, a pointer the call uses is missing
 * (`vertices` / `faces` may be NULL only when V / F is 0, and dgs_mesh_topology never reads `vertices`; count needs `counts`, the census
 * `topology`), max_vertices / max_faces < 0, an output of emit overlaps `vertices`, `faces` or the workspace, or the workspace is too
 * small or not 16-byte aligned; nothing is launched then.  V = 0 or F = 0 is valid: nothing is output (with V = 0 every face is
 * invalid, with F = 0 every vertex unreferenced), and no kernel that indexes the faces is launched. */
#ifndef DGS_MESH_REPAIR_H
#define DGS_MESH_REPAIR_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define DGS_MESH_REPAIR_COUNTS 10
#define DGS_MESH_TOPOLOGY_COUNTS 7

typedef struct DgsMeshRepairArgs {
    int64_t V, F;              /* rows of `vertices` and `faces`: V in [0, 2^30], F in [0, 2^28]                 */
    const float* vertices;     /* f32 [V, 3]; not read by dgs_mesh_topology                                      */
    const int32_t* faces;      /* i32 [F, 3]                                                                     */
    uint32_t* counts;          /* count: out uint32 [10], the order of `6 counts`                                */
    int64_t* topology;         /* census: out int64 [7], the order of `7 census`                                 */
    float* out_vertices;       /* emit: out f32 [max_vertices, 3]                                                */
    int32_t* out_faces;        /* emit: out i32 [max_faces, 3]                                                   */
    int64_t max_vertices;      /* emit: rows of `out_vertices` that may be written                               */
    int64_t max_faces;         /* emit: rows of `out_faces` that may be written                                  */
    void* workspace;           /* [dgs_mesh_repair_workspace_bytes(V, F)], 16-byte aligned; count -> emit        */
    int64_t workspace_bytes;
} DgsMeshRepairArgs;

int64_t dgs_mesh_repair_workspace_bytes(int64_t V, int64_t F);   /* 0 for unsupported sizes */
int dgs_mesh_repair_count(const DgsMeshRepairArgs* args, dgs_stream_t stream);
int dgs_mesh_repair_emit(const DgsMeshRepairArgs* args, dgs_stream_t stream);
int dgs_mesh_topology(const DgsMeshRepairArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
