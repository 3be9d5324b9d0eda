/* dgs_field.h -- C ABI of the Gaussian density field (csrc/field.hip): the occupancy grid the reference's marching cubes reads.
 *
 * Replaces GaussianModel.extract_fields of diffusionGS/models/gsrenderer/gs_core.py:786-852 (gaussian_3d_coeff :27-46,
 * build_rotation / build_scaling_rotation :112-147, the covariance activation :324-328): a Python triple loop over
 * num_blocks^3 blocks, ~15 torch ops and a host synchronisation each.  With the grid of R^3 voxels at lin[R] = linspace(-1, 1, R)
 * cut into nb^3 blocks of split = R / nb voxels per axis:
 *     members of block (xi, yi, zi): the Gaussians whose normalised centre c satisfies lo[ai] < c_a < hi[ai] STRICTLY on every axis a
 *         (lo / hi: the block's first / last coordinate -/+ block_size * relax_ratio, formed by the caller in fp32) -- a hard cut by
 *         centre that is part of the result;
 *     occ[x, y, z] = sum over the members of the voxel's block of  sigmoid(opacity) * exp(power),
 *         power = -1/2 d^T Sigma^-1 d,  d = (lin[x], lin[y], lin[z]) - c,  Sigma = (R S)(R S)^T,  R from the normalised quaternion
 *         (r, x, y, z),  S = diag(exp(scaling) * scaling_modifier * mesh_scale);  a power > 0 counts as weight 0;
 *     blocks without members are 0.
 * One deliberate deviation: Sigma^-1 is formed directly as R diag(1 / s^2) R^T; the reference inverts Sigma by the adjugate with
 * `+ 1e-24` in the determinant.  The two agree to 1e-10 of the field's maximum in fp64; ours does not lose digits to the
 * determinant's cancellation, and where the 1e-24 matters (s_x s_y s_z < ~1e-10) the reference's own result is noise.
 *
 * The call sorts the Gaussians into cells of pitch block_size (count / scan / scatter, then every Gaussian takes the rank of its
 * index inside its cell: the per-cell order is the index order whatever order the atomics arrived in), then one launch evaluates all
 * voxels: fixed summation order, plain stores.  Same inputs, same bits.  Device pointers, no allocation, no host synchronisation.
 * Returns DGS_OK or a negative DgsStatus; DGS_ERR_INVALID_ARGUMENT when N < 1, nb < 1, split < 1, R != nb * split, nb > 256, R > 2048,
 * a pointer is missing or the workspace is too small. */
#ifndef DGS_FIELD_H
#define DGS_FIELD_H

#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DgsFieldArgs {
    int32_t N;                 /* Gaussians                                                                  */
    int32_t R, nb, split;      /* voxels per axis, blocks per axis, voxels per block and axis: R = nb * split */
    const float* xyz;          /* f32 [N, 3]: NORMALISED centres (xyz - mesh_center) * mesh_scale            */
    const float* scaling;      /* f32 [N, 3]: raw (log) scales                                               */
    const float* rotation;     /* f32 [N, 4]: raw quaternions (r, x, y, z)                                   */
    const float* opacity;      /* f32 [N]: raw (logit) opacities                                             */
    float mesh_scale;          /* multiplies exp(scaling) * scaling_modifier                                 */
    float scaling_modifier;    /* 1.0 when the model has none                                                */
    const float* lin;          /* f32 [R]: voxel coordinates along one axis (the same on all three)          */
    const float* lo;           /* f32 [nb]: exclusive lower bound of a member's coordinate, per block index   */
    const float* hi;           /* f32 [nb]: exclusive upper bound                                            */
    float* occ;                /* out f32 [R, R, R], indexed [x, y, z]; every element is written             */
    void* workspace;           /* [dgs_gaussian_field_workspace_bytes(N, nb)], 16-byte aligned               */
    int64_t workspace_bytes;
} DgsFieldArgs;

int64_t dgs_gaussian_field_workspace_bytes(int32_t N, int32_t nb);
int dgs_gaussian_field(const DgsFieldArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
