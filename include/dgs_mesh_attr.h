/* dgs_mesh_attr.h -- C ABI of the mesh attributes (csrc/mesh_attr.hip): the Gaussians' density, its gradient and a density-weighted
 * mean of a per-Gaussian attribute (the colour), evaluated at query points (the mesh's vertices) instead of at voxels.
 *
 * The reference's extract_mesh returns an uncoloured trimesh.Trimesh; this is what gives the mesh of extract_mesh its vertex
 * colours and shading normals without taking the Gaussians to the host.
 *
 * Definition (order-free where it can be, with the summation order fixed where it cannot).  Inputs: the Gaussians as DgsFieldArgs
 * takes them (N, normalised centres xyz, raw scaling / rotation / opacity, mesh_scale, scaling_modifier), attr f32 [N, 3] (any three
 * numbers per Gaussian), nb in [1, 256], reach in [0, 8], points f32 [V, 3] in the same normalised cube.
 *   cell        of a coordinate x on the grid of pitch 2 / nb over [-1, 1], in fp32:  t = floor((x + 1) * (0.5f * (float)nb));
 *               cell = 0 if not t >= 0 (a NaN goes here), nb - 1 if t > nb - 1, else (int)t.  Clamped and monotone.  The cell of a
 *               Gaussian is that of its normalised centre: the key dgs_gaussian_field sorts by.
 *   members     of a point p: the Gaussians whose cell (cx, cy, cz) satisfies |cx - cell(p_x)| <= reach, |cy - cell(p_y)| <= reach and
 *               |cz - cell(p_z)| <= reach (the window, clipped to the grid).  No floating-point comparison beyond `cell`; a point
 *               outside the cube uses the clamped border cell.
 *   record      of Gaussian i: centre c_i, o_i = sigmoid(opacity_i) and (A, B, C, D, E, F) of -1/2 Sigma^-1 with the off-diagonal
 *               coefficients doubled, Sigma^-1 = R diag(1 / s^2) R^T, s = exp(scaling) * scaling_modifier * mesh_scale, R of the
 *               normalised quaternion (r, x, y, z); formed in fp64 and rounded once to fp32 (dgs_field.h).
 *   per member  d = p - c_i;  power = A dx^2 + D dy^2 + F dz^2 + B dx dy + C dx dz + E dy dz;
 *               w_i = 0 if power > 0, else exp(max(power, -126));  t_i = o_i * w_i;
 *               grad power_i = (2A dx + B dy + C dz,  B dx + 2D dy + E dz,  C dx + E dy + 2F dz).
 *   outputs     density[V]     = sum t_i
 *               attr_out[V, 3] = (sum t_i attr_i) / density where density > 0, otherwise exactly 0
 *               gradient[V, 3] = sum t_i grad power_i: the un-normalised gradient of the density; its NEGATIVE points out of the
 *                                object, the side the faces of dgs_marching_cubes turn their normals to.
 *               Each output pointer is optional, at least one must be given; an output is the same bytes whichever others are asked for.
 *   order       member cells in ascending (cx, cy, cz), ascending Gaussian index inside a cell; one fp32 accumulator per output
 *               component, plain adds (t_i attr_i and t_i grad power_i are rounded products, then added), a plain store per output.
 * So the same inputs give the same bytes, and a point's outputs depend neither on which other points are in the call nor on their
 * order.  A point with a coordinate that is not finite gets unspecified values (its cell is still a valid one: nothing is read or
 * written out of range) and changes no other point's output.
 *
 * The call sorts the Gaussians into the cells exactly as dgs_gaussian_field does (the same kernels), sorts `attr` along with the
 * records, bins the points into the same cells, and evaluates in one launch.  Device pointers, no allocation, no host synchronisation,
 * every launch on the caller's stream.
 *
 * Returns DGS_OK or a negative DgsStatus.  DGS_ERR_INVALID_ARGUMENT, decided on the host before anything is launched, when: args is
 * NULL; N < 1; nb outside [1, 256]; reach outside [0, 8]; V < 0 or V > 2^30; and, when V > 0: xyz, scaling, rotation, opacity, attr,
 * points or workspace is NULL, all three outputs are NULL, the workspace is not 16-byte aligned or workspace_bytes is less than
 * dgs_mesh_attributes_workspace_bytes(N, nb, V).  V == 0 with valid N, nb and reach returns DGS_OK and launches nothing. */
#ifndef DGS_MESH_ATTR_H
#define DGS_MESH_ATTR_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DgsMeshAttrArgs {
    int64_t V;                 /* query points, in [0, 2^30]                                                  */
    int32_t N;                 /* Gaussians                                                                  */
    int32_t nb;                /* cells per axis, pitch 2 / nb over [-1, 1], in [1, 256]                     */
    int32_t reach;             /* cells on either side of a point's cell, in [0, 8]                          */
    float mesh_scale;          /* multiplies exp(scaling) * scaling_modifier                                 */
    float scaling_modifier;    /* 1.0 when the model has none                                                */
    const float* xyz;          /* f32 [N, 3]: NORMALISED centres (xyz - mesh_center) * mesh_scale            */
    const float* scaling;      /* f32 [N, 3]: raw (log) scales                                               */
    const float* rotation;     /* f32 [N, 4]: raw quaternions (r, x, y, z)                                   */
    const float* opacity;      /* f32 [N]: raw (logit) opacities                                             */
    const float* attr;         /* f32 [N, 3]: the per-Gaussian attribute (RGB)                               */
    const float* points;       /* f32 [V, 3]: query points in the normalised cube                            */
    float* density;            /* out f32 [V], or NULL                                                       */
    float* attr_out;           /* out f32 [V, 3], or NULL                                                    */
    float* gradient;           /* out f32 [V, 3], or NULL                                                    */
    void* workspace;           /* [dgs_mesh_attributes_workspace_bytes(N, nb, V)], 16-byte aligned           */
    int64_t workspace_bytes;
} DgsMeshAttrArgs;

int64_t dgs_mesh_attributes_workspace_bytes(int32_t N, int32_t nb, int64_t V);   /* 0 for unsupported sizes */
int dgs_mesh_attributes(const DgsMeshAttrArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
