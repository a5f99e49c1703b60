/* m2t_wavelet.h -- the wavelet-domain loss term of libm2t.so: an L1 (or Charbonnier) on the bands of an undecimated 2-D wavelet
 * transform, with its gradient, and the transform alone; in HIP.
 *
 * A fifteenth header on the same library, under the conventions of m2t.h and m2t_gmsd.h (extern "C", raw device pointers, a
 * hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the fourteen older
 * headers are unchanged.  Every entry only launches: no allocation, no upload, no host synchronisation; they may sit inside a stream
 * capture.  The filter taps and the band weights are HOST arrays, read at call time and passed on to the kernels by value.
 *
 * What it adds: M2Trans moves between its three scales through a Haar DWT / IWT; the criteria of the loss table are pixel-wise,
 * whole-image statistics, a global spectrum or VGG features.  A loss on the detail bands of a stationary wavelet transform is local in
 * space and in scale at once, and a smooth output cannot pay it off.
 *
 * Definition, per image b and channel ch (C is 1 or 3); R = data range; everything after the fp32 inputs is fp64:
 *   difference  d = c(x) / R - y / R, c(t) = clamp(t, 0, R) when the clamp is on and t otherwise (each division is a multiplication by
 *               the fp64 reciprocal of R); y is never clamped.
 *   filters     an analysis pair lo[0 .. L-1], hi[0 .. L-1], 2 <= L <= 8.  The host layer knows two names:
 *               "haar": lo = (1/2, 1/2), hi = (1/2, -1/2);
 *               "db2":  with s = sqrt(3), lo = ((1+s)/8, (3+s)/8, (3-s)/8, (1-s)/8), hi[k] = (-1)^k lo[L-1-k];
 *               the orthonormal filters divided by sqrt(2): sum lo = 1, sum hi = 0, the transform is a tight frame
 *               (sum_bands ||c||^2 = ||d||^2).  Nothing is assumed about any other pair.
 *   cascade     a-trous, J levels, 1 <= J <= 3, periodic borders.  With s_j = 2^(j-1) a 1-D pass along an axis of length N is
 *               out[n] = sum_k f[k] * in[(n + k s_j) mod N], k ascending from 0.0 with separate multiply and add.  a_0 = d; level j
 *               takes the row pass (along W) of a_{j-1} with lo and with hi, then the column pass (along H) of each:
 *               LL_j = lo_col(lo_row), LH_j = hi_col(lo_row), HL_j = lo_col(hi_row), HH_j = hi_col(hi_row);  a_j = LL_j.
 *               Bands are indexed (LH_1, HL_1, HH_1, ..., LH_J, HL_J, HH_J, LL_J): 3 J + 1 bands of H x W coefficients; nothing is
 *               decimated.
 *   term        rho(c) = |c| for eps = 0 and sqrt(c^2 + eps^2) for eps > 0 (the reference's Charbonnier form, losses.py:295, with
 *               eps^2 in place of 1e-6);  value = scale * sum_bands w_band * sum_{b, ch, pixels} rho(c_band), the bands ascending;
 *               scale = 1 / (B C H W) for the mean.  Default weights: 1 for every detail band, 0 for LL_J.
 * Gradient, with respect to x only:  psi_band = w_band * rho'(c_band), rho'(c) = sign(c) with sign(+-0) = 0 for eps = 0 and
 *   c / sqrt(c^2 + eps^2) otherwise.  The adjoint of a pass is out[n] = sum_k f[k] * in[(n - k s_j) mod N].  abar_J = psi_LL; for
 *   j = J .. 1:  rl = loT_col(abar_j) + hiT_col(psi_LH_j);  rh = loT_col(psi_HL_j) + hiT_col(psi_HH_j);
 *   abar_{j-1} = loT_row(rl) + hiT_row(rh)  (each pass a sum of its own, the two then added; an absent band adds nothing);
 *   d value / d x = (scale * (1 / R)) * [0 <= x <= R] * abar_0 (the ends of the range pass; the mask only when the clamp is on).
 *   Where d is exactly 0 over a coefficient's whole support the coefficient is exactly 0; a gradient value of exactly 0 leaves the
 *   destination's bits alone.
 *
 * A band of weight 0 costs no rho and no adjoint pass, and levels above the highest weighted one are not computed.
 * Sizes: H, W >= (L - 1) * 2^(J-1) + 1 (a tap index wraps at most once), B * C <= 65535; anything else is M2T_ERR_ARG before any
 * launch.  Arithmetic: fp64 between the fp32 inputs and the one fp32 rounding of each gradient value (each coefficient of m2t_swt2);
 * partial sums are folded in a fixed order, no atomics, every output element is written by exactly one thread: two runs are
 * bit-identical, and the result does not depend on the scratch's previous contents. */
#ifndef M2T_WAVELET_H
#define M2T_WAVELET_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Bytes of device scratch the three entries below need for [B,C,H,W]: two fp64 planes for the cascade, one per band for psi, and the
 * partial sums of the 32 x 32 tiles; (3 J + 3) B C H W doubles and a little.  No initialisation needed; a 16-byte aligned address
 * lets the kernels take 16-byte pieces.  0 for an unsupported shape: levels outside 1 .. 3, taps outside 2 .. 8, C other than 1 or
 * 3, B < 1 or B * C > 65535, H or W below (taps - 1) * 2^(levels - 1) + 1. */
size_t m2t_wavelet_loss_scratch_bytes(int B, int C, int H, int W, int levels, int taps);

/* The forward transform alone (behind losses.swt2).  x [B,C,H,W] float32 on the device with image stride x_image_stride, channel
 * stride x_image_stride / C and row stride x_row_stride (elements), taken as it is (d = x: no range, no clamp); out float32
 * [B,C,3 levels + 1,H,W] contiguous, each value ONE fp32 rounding of the fp64 coefficient, the bands in the order above.
 * lo, hi: host double[taps].  scratch: m2t_wavelet_loss_scratch_bytes(B, C, H, W, levels, taps) bytes.  M2T_ERR_ARG: a null
 * argument, a bad filter / level count, an unsupported shape, strides that do not hold the image. */
int m2t_swt2(const float* x, int B, int C, int H, int W, long long x_image_stride, int x_row_stride, const double* lo, const double* hi,
             int taps, int levels, float* out, void* scratch, void* stream);

/* The plan-free loss (behind losses.wavelet_loss / WaveletLoss).  x as above, y contiguous [B,C,H,W]; with the definition above for
 * R = data_range, x clamped to [0, data_range] first when clamp != 0:
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum_bands w_band S_band),  S_band = sum rho(c_band)
 *   per_band_out[band] = S_band                       double[3 levels + 1] on the device, or NULL; 0 for a band of weight 0
 *   gx_add[q]  += (float)(d value / d x[q])           x's strides; where clamp != 0 and x[q] is outside [0, data_range], and where
 *                 the value is exactly 0, the element keeps its bits; elements outside [H,W] are never touched; NULL = value only
 *                 (no psi planes, no backward launches).
 * lo, hi: host double[taps]; band_weights: host double[3 levels + 1], finite, >= 0, not all 0, or NULL for the default (1 for every
 * detail band, 0 for LL); eps finite, >= 0.  scratch as above.  M2T_ERR_ARG: a null x / y / lo / hi / loss_out / scratch, a bad
 * filter, level count, weight vector or eps, an unsupported shape, data_range not a finite number > 0, scale not finite, strides that
 * do not hold the image. */
int m2t_wavelet_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                            float data_range, int clamp, double scale, const double* lo, const double* hi, int taps, int levels,
                            const double* band_weights, double eps, float* gx_add, float* loss_out, double* per_band_out, int accumulate,
                            void* scratch, void* stream);

/* The same routine on the forward's pre-clamp output (rgb_range = R, the clamp on), adding into the seed that the immediate pixel
 * loss or the output-gradient setter of m2t.h materialised; exactly 0 in the reflect padding; loss_out as above with
 * scale = weight / divisor.  divisor = the GLOBAL number of coefficients per band, world * accum * B * 3 * Hs * Ws, so that rank
 * shards and micro-batches sum to weight * the global mean.  scratch: m2t_wavelet_loss_scratch_bytes(B, 3, Hs, Ws, levels, taps).
 * State rules of m2t_ssim_loss: M2T_ERR_STATE without a forward with saved activations, without a seed, or after a deferred pixel
 * loss.  M2T_ERR_ARG: a null argument, a bad rgb_range / divisor / weight, a bad filter, level count, weight vector or eps, an SR
 * side below (taps - 1) * 2^(levels - 1) + 1. */
int m2t_wavelet_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, const double* lo, const double* hi,
                     int taps, int levels, const double* band_weights, double eps, float* loss_out, int accumulate, void* scratch,
                     void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
