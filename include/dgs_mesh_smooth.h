/* dgs_mesh_smooth.h -- C ABI of the mesh smoothing on the device (csrc/mesh_smooth.hip): Taubin's lambda | mu passes of the uniform
 * umbrella operator over a face-incidence list.
 *
 * The reference's clean_mesh and decimate_mesh end with pymeshlab's isotropic remeshing (a sequential edge flip / split / collapse loop
 * whose result depends on the order of its operations; it stays third-party) and carry ms.apply_coord_taubin_smoothing() as the
 * commented alternative.  Taubin smoothing has an order-free definition, stated here, and does not shrink the object the way plain
 * Laplacian smoothing does.  The vertices move, the faces stay as they are; the mesh stays on the device.
 *
 * Definition (order-free, so the result can be pinned bit for bit).  Inputs: vertices f32 [V, 3], faces i32 [F, 3], lambda and mu as
 * doubles, iterations >= 0, optionally fixed u8 [V].
 *   valid       A face is VALID iff its three indices lie in [0, V).  An invalid face is never dereferenced; it is ignored and counted.
 *   null        A valid face with two equal indices is NULL; it is ignored and counted (it would make a vertex its own neighbour).
 *   incidence   For a vertex v, c_v is the number of valid, non-null faces that name it; duplicated faces count as often as they
 *               occur.  Its neighbour multiset N_v holds the two other corners of each such face: 2 c_v entries.  On a closed manifold
 *               mesh every neighbour appears exactly twice, and the mean over N_v is the uniform umbrella operator, what MeshLab's
 *               filter uses with the cotangent weights off.  Border vertices get no special treatment (VCG moves them along the
 *               border only): an open mesh shrinks at its border.
 *   moving      v MOVES iff 1 <= c_v <= 16384 and (fixed is NULL or fixed[v] == 0).  Every other vertex keeps its input bytes through
 *               every pass (and still is a neighbour of the vertices that name it).  Two kinds of them are counted: the
 *               unreferenced ones (c_v = 0) and the ones above the cap (c_v > 16384).
 *   pass(w)     Jacobi: every read comes from the pass's input.  For a moving vertex and each axis k:
 *                   Q(x)  = llrint(min(max((double)x, -32768.0), 32768.0) * 4294967296.0)        fixed point, 2^-32
 *                   S_k   = the int64 sum of Q(p_u,k) over the entries u of N_v: at most 2^15 * 2^47 = 2^62 in magnitude, the same
 *                           in every order
 *                   m_k   = (double)S_k / ((double)(2 c_v) * 4294967296.0)
 *                   p'_k  = (float)((double)p_k + w * (m_k - (double)p_k))
 *               every fp64 operation rounded on its own (no fused multiply-add, no reassociation), every conversion round to nearest
 *               even.  A pass with w == 0 is the identity and is not run (so -0.0 stays -0.0).
 *   smoothing   `iterations` times: pass(lambda), then pass(mu).  MeshLab's defaults are 0.5, -0.53 and 10.  mu = 0 gives plain
 *               Laplacian smoothing; iterations = 0, or lambda = mu = 0, returns the input bytes.
 *   counts      uint32 [4] = {invalid faces, null faces, vertices over the incidence cap, unreferenced vertices}.
 * Coordinates that are not finite give unspecified positions and never an access out of range: no address depends on a coordinate.
 * Coordinates beyond +-32768 enter the means clamped.
 *
 * Invariance.  Renaming the vertices (faces and `fixed` renumbered to match) permutes the output rows and changes no byte.  Permuting
 * the faces changes nothing.  Rotating or reversing the corners of a face changes nothing.
 *
 * What this is not: no border handling, no cotangent weights, no remeshing, no repair of non-manifold edges or vertices: that is
 * dgs_mesh_repair.h (dgs_mesh_repair_count / _emit), which extract_mesh(repair=True) runs in front of this.
 *
 * One call (the output always has V rows): device pointers, no allocation, no host synchronisation.  Built once per call: c_v by
 * integer atomic adds per vertex, an exclusive scan of the segment lengths (2 c_v for a moving vertex; the vertices that do not move
 * need no segment), and a flat neighbour array of at most 6 F int32 entries filled through per-vertex atomic cursors.  The order inside
 * a segment depends on the order in which the faces arrive; the pass sums integers, so nothing that is output does.  Those are the only
 * atomics.  Each pass is a pure gather from one buffer into the other (the workspace and out_vertices in turn, arranged so that the
 * last pass writes out_vertices): a vertex of c_v <= 48 takes a thread, one of c_v > 48 a wave whose lanes stride over the segment and
 * add their integers up.  The same input gives the same bytes in every run.
 *
 * Limits: V in [0, 2^30], F in [0, 2^29] (6 F must fit 32 bits), iterations in [0, 2^20].
 *
 * Returns DGS_OK or a negative DgsStatus; DGS_ERR_INVALID_ARGUMENT when V, F or iterations is outside its limits, lambda or mu is not
 * finite, a pointer the call uses is missing (`vertices` / `out_vertices` may be NULL only when V is 0, `faces` only when F is 0;
 * `fixed` and `counts` may always be NULL), out_vertices overlaps vertices, or the workspace is too small or not 16-byte aligned.
 * V = 0 or F = 0 is valid: the vertices come back as they are (with F = 0 all V are unreferenced), and no kernel that indexes the faces
 * is launched. */
#ifndef DGS_MESH_SMOOTH_H
#define DGS_MESH_SMOOTH_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DgsMeshSmoothArgs {
    int64_t V, F;              /* rows of `vertices` and `faces`: V in [0, 2^30], F in [0, 2^29]                 */
    const float* vertices;     /* f32 [V, 3]                                                                     */
    const int32_t* faces;      /* i32 [F, 3]                                                                     */
    const uint8_t* fixed;      /* u8 [V] or NULL: a vertex with a non-zero entry keeps its input bytes           */
    double lambda, mu;         /* the weights of the two passes of an iteration                                  */
    int32_t iterations;        /* in [0, 2^20]                                                                   */
    uint32_t* counts;          /* out uint32 [4] = {invalid faces, null faces, over the cap, unreferenced}, or NULL */
    float* out_vertices;       /* out f32 [V, 3]; must not overlap `vertices`                                    */
    void* workspace;           /* [dgs_mesh_smooth_workspace_bytes(V, F)], 16-byte aligned                       */
    int64_t workspace_bytes;
} DgsMeshSmoothArgs;

int64_t dgs_mesh_smooth_workspace_bytes(int64_t V, int64_t F);   /* 0 for unsupported sizes */
int dgs_mesh_smooth(const DgsMeshSmoothArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
