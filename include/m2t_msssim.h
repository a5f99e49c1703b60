/* m2t_msssim.h -- the multi-scale structural loss term of libm2t.so: 1 - MS-SSIM with its gradient, in HIP.
 *
 * A fourth header on the same library, under the conventions of m2t.h, m2t_spectral.h and m2t_resize.h (extern "C", raw device
 * pointers, a hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the
 * three older headers are unchanged.  Every entry only launches: no allocation, no upload, no host synchronisation; they may sit
 * inside a stream capture.
 *
 * What it replaces: the reference imports MultiScaleSSIMLoss from piq next to the pixel criteria (losses.py:8); L1 + MS-SSIM is
 * the structural recipe of Zhao et al., "Loss functions for image restoration with neural networks".
 *
 * Definition, per image b and channel c (the pytorch_msssim.ms_ssim / piq.multi_scale_ssim form):
 *   x_0 = clamp(pre, 0, R) / R,  y_0 = hr / R  (data_range 1);  five levels l = 0 .. 4, weights w = (0.0448, 0.2856, 0.3001, 0.2363,
 *   0.1333);  window (the 11 fp32 taps torch builds for sigma 1.5, widened to fp64; VALID), K = (0.01, 0.03) and m1, m2, s1, s2, s12,
 *   A1, A2, B1, B2 as for m2t_ssim_loss of m2t.h;
 *   v_l = mean over the map of A2 / B2 (contrast-structure) for l < 4,  v_4 = mean over the map of A1 A2 / (B1 B2) (SSIM);
 *   x_{l+1} = avg_pool2d(x_l, kernel 2, stride 2, padding (H_l % 2, W_l % 2), zeros counted): side floor(n / 2) + n % 2, every output
 *   the sum of the in-image members of its 2 x 2 cell times 1 / 4, the cells starting at index -1 on an odd side; y likewise;
 *   M_bc = prod_l max(v_l, 0)^{w_l};   term = weight * (1 - mean_{b,c} M_bc).
 * Gradient: with every v_l > 0, dM / dx_l(q) = (w_l M / v_l) / n_l * d sum(map_l) / dx_l(q) (n_l map entries), carried to level 0 by
 * the adjoint of the pooling (each fine pixel takes 1 / 4 of its one parent), through the clamp mask of the pixel losses (ends of
 * [0, R] included in the pass band) and 1 / R.  Where any v_l <= 0:  M_bc = 0 and that (image, channel) adds NOTHING to the
 * gradient -- its destination bits stay as they were (torch's autograd forms 0 * inf there: a documented deviation).
 *
 * Sizes: min(H, W) > 160 (the packages' own assertion, (11 - 1) * 2^4); anything smaller is M2T_ERR_ARG before any launch.
 * Arithmetic: the pooled levels are fp64 (a level-l value is a sum of at most 4^l fp32 numbers times a power of two); everything
 * between the fp32 inputs and the one fp32 rounding of each gradient value is fp64; partial sums are folded in a fixed order, no
 * atomics, every output element is written by exactly one thread: two runs are bit-identical.
 * Parity with pytorch_msssim / piq themselves is unpinned (neither is installed where this library is built); the definition is
 * pinned by an fp64 restatement and torch autograd. */
#ifndef M2T_MSSSIM_H
#define M2T_MSSSIM_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Bytes of device scratch the two loss entries need for [B,C,H,W]: the per-(b,c) record, the partial sums, both fp64 pyramids
 * (levels 1 .. 4) and the fp64 gradient levels 1 .. 4.  No initialisation needed.  0 for min(H, W) <= 160, B or C < 1, or
 * B * C > 65535. */
size_t m2t_msssim_loss_scratch_bytes(int B, int C, int H, int W);

/* Where a region of that scratch starts (bytes), for audits and tests; (size_t)-1 for an unsupported shape, region or level.
 *   region 0: the record, 12 doubles per (b,c): c_0 .. c_4 (= w_l M / (v_l n_l), 0 under the zero rule), M, alive (1 / 0), v_0 .. v_4
 *   region 1: the partial sums of level `level` (0 .. 4), [B*C][tiles]
 *   region 2 / 3: level `level` (1 .. 4) of the x / y pyramid, contiguous [B*C][H_l][W_l] doubles, UN-normalised (pooled
 *                 clamp(x, 0, R), pooled y: exact, and equal to R times the levels of the definition)
 *   region 4: the gradient of M_bc with respect to the normalised level `level` (1 .. 4), the same shape (written only by a call
 *             with gx_add != NULL, and only for the (b,c) the zero rule does not silence) */
size_t m2t_msssim_loss_scratch_offset(int B, int C, int H, int W, int region, int level);

/* The plan-free loss (behind losses.ms_ssim_loss / MSSSIMLoss and metrics.ms_ssim_device).  x [B,C,H,W] float32 on the device with
 * image stride x_image_stride, channel stride x_image_stride / C and row stride x_row_stride (elements); y contiguous [B,C,H,W].
 * With M_bc as above for R = data_range, x clamped to [0, data_range] first when clamp != 0:
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum_bc (1 - M_bc))          (scale = 1 / (B C) for the mean)
 *   per_channel_out[b * C + c] = M_bc                                      double[B*C] on the device, or NULL
 *   gx_add[q]  += (float)(-scale / data_range * dM_bc / dx_0[q])           x's strides; where clamp != 0 and x[q] is outside
 *                 [0, data_range], or the zero rule holds for (b,c), the element is left alone; elements outside [H,W] are never
 *                 touched; NULL = value only (no gradient launches).
 * scratch: m2t_msssim_loss_scratch_bytes(B, C, H, W) bytes.  M2T_ERR_ARG: a null x / y / loss_out / scratch, B * C outside
 * 1 .. 65535, min(H, W) <= 160, data_range not a finite number > 0, strides that do not hold the image. */
int m2t_msssim_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                           float data_range, int clamp, double scale, float* gx_add, float* loss_out, double* per_channel_out,
                           int accumulate, void* scratch, void* stream);

/* The same routine on the forward's pre-clamp output (rgb_range = R, the clamp on), adding into the seed that the immediate pixel
 * loss or the output-gradient setter of m2t.h materialised; exactly 0 in the reflect padding; loss_out as above with
 * scale = weight / divisor.  divisor = the GLOBAL number of (image, channel) pairs, world * accum * B * 3, so that rank shards and
 * micro-batches sum to weight * (1 - the global mean MS-SSIM).  scratch: m2t_msssim_loss_scratch_bytes(B, 3, Hs, Ws).  State rules
 * of m2t_ssim_loss: M2T_ERR_STATE without a forward with saved activations, without a seed, or after a deferred pixel loss.
 * M2T_ERR_ARG: a null argument, an SR side <= 160, a bad rgb_range / divisor / weight. */
int m2t_msssim_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, float* loss_out, int accumulate,
                    void* scratch, void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
