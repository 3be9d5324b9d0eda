/* dgs_lpips.h -- C ABI of LPIPS-VGG on the device (csrc/lpips.hip): what `lpips.LPIPS(net="vgg")` (version 0.1,
 * lpips=True, spatial=False, eval mode) computes for two image batches, in fp32, with a 3x3 convolution on the f32-input MFMA, and
 * the gradient of that number with respect to the images ("The input gradient" below).  The network is frozen: no weight gradient.
 *
 * The network.  in0, in1: f32 [n, 3, H, W] in (-1, 1).
 *   scaling     s = (x - shift[c]) / scale[c], shift = (-.030, -.088, -.188), scale = (.458, .448, .450) (given by the caller).
 *   features    thirteen 3x3 convolutions, zero padding 1 (of the SCALED input), bias, ReLU; Cin -> Cout:
 *               3->64, 64->64, pool, 64->128, 128->128, pool, 128->256, 256->256, 256->256, pool, 256->512, 512->512, 512->512,
 *               pool, 512->512, 512->512, 512->512.  pool = 2x2 maximum, stride 2, odd sizes floored.
 *   taps        f_k, k = 0..4: the ReLU output of convolutions 2, 4, 7, 10, 13 (C = 64, 128, 256, 512, 512), at
 *               (H, W), (H/2, W/2), ... , (H/16, W/16), each division floored.
 *   per tap     fh = f / (sqrt(sum_c f^2) + 1e-10) per pixel;  d_k = mean_{h,w} sum_c lin_k[c] (fh0 - fh1)^2, lin_k >= 0.
 *   result      out[n] = d_0 + d_1 + d_2 + d_3 + d_4 (added in this order).
 *
 * Layouts.  Inside the library an activation is CHANNELS-LAST: f32 [N, H, W, C], element (n, h, w, c) at ((n H + h) W + w) C + c.
 *   packed weights   A convolution takes its weights as the GEMM operand B[k][co]: f32 [Kp][Cp], row-major, with
 *                    k = (3 ky + kx) Cin + ci, Kp = 9 Cin rounded up to 32, Cp = Cout rounded up to 64, and
 *                    B[k][co] = w[co][ci][ky][kx] for a torch weight w [Cout, Cin, 3, 3]; every padding entry is 0.
 *                    dgs_conv3x3_packed_floats gives Kp Cp; dgs_lpips_pack_weights fills it from ANY such tensor (so the data
 *                    gradient of a convolution, the same convolution on flipped, transposed weights, can use the same kernel).
 *
 * Arithmetic.  An output element of a convolution is ONE chain of fused multiply-adds over k = 0, 1, ..., 9 Cin - 1 in this order,
 * starting from 0 (v_mfma_f32_32x32x2_f32 executes exactly that chain; a tap outside the image contributes fma(0, w, acc) = acc); the
 * bias is added after the chain, then the ReLU.  The order does not depend on where the element lies in a tile, in the image or in
 * the batch.  The tap kernel sums the channels of a pixel lane by lane (lane l takes c = l, l + 64, ...) and then in a fixed
 * butterfly, the pixels of an image thread by thread (thread t takes p = t, t + 256, ...) and then in a fixed tree; no floating-point
 * sum uses an atomic.  Consequences: the same input gives the same bytes; a pair's result does not depend on the other pairs of the
 * call, on its position in the batch or on the chunking; lpips(x, x) is exactly 0.
 *
 * The input gradient.  Backward of one chunk, from the last tap down, with y_i the ReLU output of convolution i (all thirteen kept
 * from the chunk's forward; pool outputs are not kept):
 *   tap          with s = sum_c f_c^2, r = sqrt(s), n = r + 1e-10, e_c = f0_c / n0 - f1_c / n1, A0 = sum_c lin_c e_c f0_c (A1 alike):
 *                g0_c = (2 / (H W)) (lin_c e_c / n0 - f0_c A0 / (n0^2 r0)),  g1_c = (2 / (H W)) (-lin_c e_c / n1 + f1_c A1 / (n1^2 r1)).
 *                An element whose own f is 0 is written as 0 (that is the ReLU's mask), so 0 / 0 at a pixel whose vector is all
 *                zero is never evaluated: torch's autograd returns NaN at such a pixel, this call returns 0.
 *   convolution  dX[n,h,w,ci] = sum_{ky,kx,co} dZ[n,h-ky+1,w-kx+1,co] w[co][ci][ky][kx]: dgs_conv3x3 on w'[ci][co][ky][kx] =
 *                w[co][ci][2-ky][2-kx], whose packed operand dgs_lpips_pack_weights_transposed writes from w itself; the same
 *                kernel, the same k-ordered chain (k = (3 ky' + kx') Cout + co), with the epilogue (mask > 0 ? acc : 0) + add.
 *   pool         an element receives its window's dY if it is the FIRST maximum of the window in (row, column) order (`>` against
 *                the running maximum, as torch routes it; a NaN is never a maximum here), every other element and the last row or
 *                column of an odd size 0; then (x > 0 ? routed : 0) + add with x the pooled ReLU output.
 *   sequence     dz_i = (y_i > 0) ? (downstream_i + tap_i) : 0;  dx[n,c,h,w] = ds[n,h,w,c] / scale[c].
 * The channel sums of the tap use the forward's lane order and butterfly; an output element of any of these kernels depends on its
 * own pixel's (window's, receptive field's) data only, nothing is accumulated across pairs and no float atomic is used.  Consequences:
 * the same input gives the same bytes; a pair's gradient does not depend on the other pairs, on its position or on the chunk size;
 * grad0 is the same bytes whether grad1 was asked for or not; the gradient of lpips(x, x) is exactly 0.
 * The first layer's data gradient (64 -> 3) runs with its 3 output channels padded to 64, about twenty times the work its shape
 * needs: it costs what one 64 -> 64 layer costs, and there is no dedicated kernel for it.
 *
 * Calls take device pointers and a stream, allocate nothing and never synchronise with the host.
 *
 * Limits: every dimension >= 1; N H W < 2^31 - 256 for a convolution; N H W C < 2^40.  dgs_lpips_forward needs H >= 16 and
 * W >= 16 (the last tap would be empty otherwise) and H W <= 2^20.
 *
 * Every function returns DGS_OK or a negative DgsStatus; DGS_ERR_INVALID_ARGUMENT for a size outside the limits, a missing pointer
 * or a workspace that is too small or not 16-byte aligned. */
#ifndef DGS_LPIPS_H
#define DGS_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#include "dgs_raster.h" /* DgsStatus, dgs_stream_t */

#ifdef __cplusplus
extern "C" {
#endif

#define DGS_LPIPS_CONVS 13
#define DGS_LPIPS_TAPS 5

typedef struct DgsConv3x3Args {
    int32_t N, H, W, Cin, Cout;
    const float* x;        /* f32 [N, H, W, Cin], channels-last                                   */
    const float* weights;  /* packed f32 [Kp][Cp] (above), 16-byte aligned                        */
    const float* bias;     /* f32 [Cout] or NULL                                                  */
    int32_t relu;          /* non-zero: max(., 0) after the bias                                  */
    float* y;              /* out f32 [N, H, W, Cout], channels-last; must not overlap x          */
} DgsConv3x3Args;

typedef struct DgsMaxPool2x2Args {
    int32_t N, H, W, C;
    const float* x;        /* f32 [N, H, W, C]                                                    */
    float* y;              /* out f32 [N, H / 2, W / 2, C] (floored); nothing is written when H or W is 1 */
} DgsMaxPool2x2Args;

typedef struct DgsLpipsPackArgs {
    int32_t Cin, Cout;
    const float* w;        /* f32 [Cout, Cin, 3, 3], torch's layout                               */
    float* packed;         /* out f32 [dgs_conv3x3_packed_floats(Cin, Cout)]                      */
} DgsLpipsPackArgs;

typedef struct DgsLpipsTapArgs {
    int32_t N, H, W, C;
    const float* f0;       /* f32 [N, H, W, C] features of the first images                       */
    const float* f1;       /* f32 [N, H, W, C] features of the second images                      */
    const float* lin;      /* f32 [C]                                                             */
    float* out;            /* out f32 [N * out_stride]: d of pair n at out[n * out_stride]        */
    int32_t out_stride;    /* >= 1                                                                */
    float* workspace;      /* f32 [N H W]                                                         */
} DgsLpipsTapArgs;

typedef struct DgsLpipsForwardArgs {
    int32_t N, H, W;
    const float* x0;       /* f32 [N, 3, H, W] (torch's layout), in (-1, 1)                       */
    const float* x1;       /* f32 [N, 3, H, W]                                                    */
    const float* shift;    /* f32 [3]                                                             */
    const float* scale;    /* f32 [3]                                                             */
    const float* conv_w[DGS_LPIPS_CONVS];  /* packed weights of the thirteen convolutions         */
    const float* conv_b[DGS_LPIPS_CONVS];  /* f32 [Cout] each                                     */
    const float* lin[DGS_LPIPS_TAPS];      /* f32 [C_k] each                                      */
    float* out;            /* out f32 [N]                                                         */
    float* per_tap;        /* out f32 [N, 5] (d_k of every pair) or NULL                          */
    float* const* features;/* NULL, or a HOST table of five device pointers; entry k receives f32 [2, N, H_k, W_k, C_k]:
                              the tap's features of x0 ([0]) and of x1 ([1]), channels-last       */
    int32_t chunk;         /* pairs pushed through the network at once (as one batch of 2 chunk images); 0: the largest the
                              workspace of dgs_lpips_workspace_bytes holds.  Changes no byte of any output. */
    void* workspace;       /* [dgs_lpips_workspace_bytes(N, H, W)], 16-byte aligned               */
    size_t workspace_bytes;
} DgsLpipsForwardArgs;

int64_t dgs_conv3x3_packed_floats(int32_t Cin, int32_t Cout);   /* Kp * Cp; 0 for sizes below 1 */
int dgs_lpips_pack_weights(const DgsLpipsPackArgs* args, dgs_stream_t stream);
int dgs_conv3x3(const DgsConv3x3Args* args, dgs_stream_t stream);
int dgs_maxpool2x2(const DgsMaxPool2x2Args* args, dgs_stream_t stream);
int dgs_lpips_tap(const DgsLpipsTapArgs* args, dgs_stream_t stream);
/* pairs per chunk that dgs_lpips_forward uses with chunk = 0: min(N, max(1, 2^19 / (H W))); 0 for unsupported sizes */
int32_t dgs_lpips_chunk(int32_t N, int32_t H, int32_t W);
/* bounded in N: it depends on min(N, dgs_lpips_chunk) only; 0 for unsupported sizes */
size_t dgs_lpips_workspace_bytes(int32_t N, int32_t H, int32_t W);
int dgs_lpips_forward(const DgsLpipsForwardArgs* args, dgs_stream_t stream);

/* ---- the input gradient ---- */

typedef struct DgsConv3x3BackwardDataArgs {
    int32_t N, H, W, Cin, Cout;   /* of the FORWARD convolution: dy has Cout channels, dx has Cin                                 */
    const float* dy;       /* f32 [N, H, W, Cout], channels-last                                  */
    const float* weights;  /* dgs_lpips_pack_weights_transposed of the forward's w: f32 [dgs_conv3x3_packed_floats(Cout, Cin)] */
    const float* mask;     /* f32 [N, H, W, Cin] or NULL: where it is not > 0 the sum is replaced by 0 (the ReLU below)         */
    const float* add;      /* f32 [N, H, W, Cin] or NULL: added after the mask; may be dx itself  */
    float* dx;             /* out f32 [N, H, W, Cin] = (mask > 0 ? sum : 0) + add; must not overlap dy */
} DgsConv3x3BackwardDataArgs;

typedef struct DgsMaxPool2x2BackwardArgs {
    int32_t N, H, W, C;
    const float* x;        /* f32 [N, H, W, C]: the pool's input                                  */
    const float* dy;       /* f32 [N, H / 2, W / 2, C]; not read when H or W is 1                 */
    int32_t relu_mask;     /* non-zero: the routed value is replaced by 0 where x is not > 0      */
    const float* add;      /* f32 [N, H, W, C] or NULL: added after the mask; may be dx itself    */
    float* dx;             /* out f32 [N, H, W, C]                                                */
} DgsMaxPool2x2BackwardArgs;

typedef struct DgsLpipsTapBackwardArgs {
    int32_t N, H, W, C;
    const float* f0;       /* f32 [N, H, W, C], >= 0 (a ReLU output)                              */
    const float* f1;       /* f32 [N, H, W, C]                                                    */
    const float* lin;      /* f32 [C]                                                             */
    float* g0;             /* out f32 [N, H, W, C]: d d[n] / d f0, 0 where f0 is 0                */
    float* g1;             /* out f32 [N, H, W, C]: d d[n] / d f1, 0 where f1 is 0; or NULL       */
} DgsLpipsTapBackwardArgs;

typedef struct DgsLpipsGradArgs {
    int32_t N, H, W;
    const float* x0;       /* as DgsLpipsForwardArgs                                              */
    const float* x1;
    const float* shift;
    const float* scale;
    const float* conv_w[DGS_LPIPS_CONVS];   /* packed weights (dgs_lpips_pack_weights)             */
    const float* conv_wt[DGS_LPIPS_CONVS];  /* the same weights through dgs_lpips_pack_weights_transposed */
    const float* conv_b[DGS_LPIPS_CONVS];
    const float* lin[DGS_LPIPS_TAPS];
    float* out;            /* out f32 [N]: the bytes dgs_lpips_forward gives                      */
    float* per_tap;        /* out f32 [N, 5] or NULL                                              */
    float* grad0;          /* out f32 [N, 3, H, W]: d out[n] / d x0[n]                            */
    float* grad1;          /* out f32 [N, 3, H, W]: d out[n] / d x1[n]; or NULL, then the backward convolutions run over the x0
                              images only (half the work); grad0 has the same bytes either way    */
    int32_t chunk;         /* pairs per pass; 0: dgs_lpips_grad_chunk.  Changes no byte of any output. */
    void* workspace;       /* [dgs_lpips_grad_workspace_bytes(N, H, W)], 16-byte aligned          */
    size_t workspace_bytes;
} DgsLpipsGradArgs;

/* w [Cout, Cin, 3, 3] -> packed [dgs_conv3x3_packed_floats(Cout, Cin)]: the operand of the convolution Cout -> Cin on
 * w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx] */
int dgs_lpips_pack_weights_transposed(const DgsLpipsPackArgs* args, dgs_stream_t stream);
int dgs_conv3x3_backward_data(const DgsConv3x3BackwardDataArgs* args, dgs_stream_t stream);
int dgs_maxpool2x2_backward(const DgsMaxPool2x2BackwardArgs* args, dgs_stream_t stream);
int dgs_lpips_tap_backward(const DgsLpipsTapBackwardArgs* args, dgs_stream_t stream);
/* pairs per chunk of dgs_lpips_forward_backward with chunk = 0: that of the forward, min(N, max(1, 2^19 / (H W))) */
int32_t dgs_lpips_grad_chunk(int32_t N, int32_t H, int32_t W);
/* Bounded in N (it depends on min(N, dgs_lpips_grad_chunk) only); 0 for unsupported sizes.  Per image of the chunk (two per pair), in
 * floats: 3 H W (the scaled input) + the thirteen ReLU outputs (270 H W for sizes divisible by 16) + 2 x 64 H W (two gradient
 * buffers) + a little per pair.  At 256^2, 8 pairs: 16 x 26.3 M floats = 1.68 GB, of which the ReLU outputs are 1.13 GB. */
size_t dgs_lpips_grad_workspace_bytes(int32_t N, int32_t H, int32_t W);
/* out[n] as dgs_lpips_forward (the same kernels, the same bytes) and its gradient with respect to x0[n] (and x1[n]), chunk by chunk:
 * forward of the chunk keeping the thirteen ReLU outputs, then backward from the last tap down */
int dgs_lpips_forward_backward(const DgsLpipsGradArgs* args, dgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
