/* m2t_gmsd.h -- the gradient-magnitude-similarity-deviation loss term of libm2t.so: GMSD with its gradient, in HIP.
 *
 * A twelfth header on the same library, under the conventions of m2t.h and m2t_vif.h (extern "C", raw device pointers, a hipStream_t
 * passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the eleven older headers are
 * unchanged.  Every entry only launches: no allocation, no upload, no host synchronisation; they may sit inside a stream capture.
 *
 * What it replaces: the reference scores a model by PSNR, SSIM, FSIM and GMSD (test.py:95-122); piq ships GMSDLoss next to the three
 * classes the reference imports (losses.py:8).  The forward exists as a metric (m2t_eval_gmsd of m2t.h, an fp32 map, untouched by
 * this header); torch autograd through sqrt(gx^2 + gy^2) gives 0 * inf = NaN wherever the image is locally flat -- the black sector
 * mask of every ultrasound frame -- so the gradient is a closed form with stated conventions.
 *
 * Definition, per image b; R = data range, T = 170 / 255^2; everything after the fp32 inputs is fp64:
 *   luminance  l(x) = (0.299 c(x_R) + 0.587 c(x_G) + 0.114 c(x_B)) / R, c(t) = clamp(t, 0, R) when the clamp is on and t otherwise
 *              (the division is a multiplication by the fp64 reciprocal of R); with one channel l = c(x) / R; y is never clamped.
 *              C is 1 or 3.
 *   pooling    hp = ceil(H / 2), wp = ceil(W / 2);  u(p) = 0.25 * ((l00 + l01) + (l10 + l11)) over the 2 x 2 cell, a cell row or
 *              column beyond the image counting as 0 (piq's zero pad to an even size, as m2t_eval_gmsd has it);  v the same of y.
 *   Prewitt    zero padding, DIFFERENCES FIRST:
 *              gx = ((u[-1,+1] - u[-1,-1]) + (u[0,+1] - u[0,-1]) + (u[+1,+1] - u[+1,-1])) / 3,
 *              gy = ((u[+1,-1] - u[-1,-1]) + (u[+1,0] - u[-1,0]) + (u[+1,+1] - u[-1,+1])) / 3  ([row, column] offsets);
 *              m = sqrt(gx^2 + gy^2), m' the same of v.  In a flat region every difference is exactly 0 in any summation order; a
 *              weighted 9-tap sum is not (an fp64 conv2d leaves about 6e-19 there, and the gradient would point along rounding noise).
 *   map        D = m^2 + m'^2 + T;  s = (2 m m' + T) / D;  accumulated is d = 1 - s = (m - m')^2 / D, FORMED THAT WAY;
 *              n = hp * wp;  var = sum d^2 / n - (sum d / n)^2 floored at 0;  GMSD_b = sqrt(var).  Summing d keeps the variance free of
 *              cancellation for near-identical images, where s is about 1.
 *   term       weight * mean_b GMSD_b.  GMSD is a distortion, 0 = identical: there is no "1 -".
 * Gradient, with respect to x only:  mu = sum s / n;  k_i = (s_i - mu) / (n GMSD_b) (formed as (sum d / n - d_i) / (n GMSD_b));
 *   rho_i = m'_i / m_i where m_i > 0, and where m_i = 0 the whole entry is 0 (there gx = gy = 0: the convention that replaces torch's NaN);
 *   a_x = k * 2 (rho - s) / D * gx,  a_y = k * 2 (rho - s) / D * gy;  dGMSD / du = the adjoint of the zero-padded Prewitt pair applied to
 *   (a_x, a_y), an entry outside the map contributing nothing;
 *   dGMSD / dx_ch(pixel) = 0.25 * w_ch / R * [0 <= x_ch <= R] * dGMSD / du(cell of the pixel) (the ends of the range pass; the mask only
 *   when the clamp is on).  An image with GMSD_b = 0 adds nothing: its gradient elements are not written at all.  Identical images give
 *   this, and so does any image with H, W <= 2, whose map is 1 x 1.
 *
 * Sizes: H, W >= 2, B <= 65535; anything else is M2T_ERR_ARG before any launch.  Arithmetic: fp64 between the fp32 inputs and the one
 * fp32 rounding of each gradient value; partial sums are folded in a fixed order, no atomics, every output element is written by
 * exactly one thread: two runs are bit-identical, and the result does not depend on the scratch's previous contents.
 * Parity with piq itself is unpinned (it is not installed where this library is built); the definition is pinned by an fp64
 * restatement, by the oracle's gmsd and by torch autograd where autograd is finite. */
#ifndef M2T_GMSD_H
#define M2T_GMSD_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Bytes of device scratch the two loss entries need for [B,C,H,W]: the per-image record (4 doubles: sum d, sum d^2, GMSD_b,
 * scale / (n GMSD_b)) and the partial sums of the 32 x 32-cell tiles.  No initialisation needed.  0 for an unsupported shape: H or W
 * below 2, C other than 1 or 3, B < 1 or B > 65535. */
size_t m2t_gmsd_loss_scratch_bytes(int B, int C, int H, int W);

/* The plan-free loss (behind losses.gmsd_loss / GMSDLoss).  x [B,C,H,W] float32 on the device with image stride x_image_stride,
 * channel stride x_image_stride / C and row stride x_row_stride (elements); y contiguous [B,C,H,W].  With GMSD_b as above for
 * R = data_range, x clamped to [0, data_range] first when clamp != 0:
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum_b GMSD_b)                (scale = 1 / B for the mean)
 *   per_image_out[b] = GMSD_b                                               double[B] on the device, or NULL
 *   gx_add[q]  += (float)(scale * dGMSD_b / dx[q])                          x's strides; where clamp != 0 and x[q] is outside
 *                 [0, data_range] the element keeps its bits; elements outside [H,W] and all elements of an image with GMSD_b = 0
 *                 are never touched; NULL = value only (no gradient launch).
 * scratch: m2t_gmsd_loss_scratch_bytes(B, C, H, W) bytes.  M2T_ERR_ARG: a null x / y / loss_out / scratch, B outside 1 .. 65535,
 * C other than 1 or 3, H or W < 2, data_range not a finite number > 0, scale not finite, strides that do not hold the image. */
int m2t_gmsd_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                         float data_range, int clamp, double scale, float* gx_add, float* loss_out, double* per_image_out,
                         int accumulate, void* scratch, void* stream);

/* The same routine on the forward's pre-clamp output (rgb_range = R, the clamp on), adding into the seed that the immediate pixel
 * loss or the output-gradient setter of m2t.h materialised; exactly 0 in the reflect padding; loss_out as above with
 * scale = weight / divisor.  divisor = the GLOBAL number of images, world * accum * B (not times 3: the luminance collapses the
 * channels), so that rank shards and micro-batches sum to weight * the global mean GMSD.  scratch:
 * m2t_gmsd_loss_scratch_bytes(B, 3, Hs, Ws).  State rules of m2t_ssim_loss: M2T_ERR_STATE without a forward with saved activations,
 * without a seed, or after a deferred pixel loss.  M2T_ERR_ARG: a null argument, an SR side < 2, a bad rgb_range / divisor / weight. */
int m2t_gmsd_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, float* loss_out, int accumulate,
                  void* scratch, void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
