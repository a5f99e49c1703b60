/* m2t_consistency.h -- LR-consistency on libm2t.so: the bicubic-down loss term with its gradient, the adjoint of the down-sampler, and
 * one iteration of back-projection, in HIP.
 *
 * An eighteenth header on the same library, under the conventions of m2t.h and m2t_gmsd.h (extern "C", raw device pointers, a
 * hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the seventeen older
 * headers are unchanged.  Every entry only launches: no allocation, no upload (the filter taps travel in the kernel arguments), no host
 * synchronisation; they may sit inside a stream capture.
 *
 * What it is for: every other criterion of the library compares SR with HR.  This one asks whether the output, degraded the way the
 * acquisition was, gives back the image that was acquired: the "dual regression" / cycle term rho(D(clamp(sr)) - lr), which needs no
 * HR; Irani-Peleg back-projection at inference; and LR-PSNR, the consistency score of the NTIRE reports.
 *
 * Definitions.
 *   D = D_s    s in {2, 3, 4}: the "down" case of m2t_resize.h.  Per axis of length n = m s, output i takes the taps j = i s + M0 + t
 *              (8 / 11 / 16 taps from M0 = -3 / -4 / -6) with the normalised weights w_t, folded by the mirror with the edge pixel
 *              repeated (period 2 n, applied modulo 2 n: a short axis reflects more than once); rows (vertical) first, then columns;
 *              everything in fp64, nothing rounded between the passes.  As matrices D x = A_H x A_W^T,
 *              A_n[i, mirror(i s + M0 + t)] += w_t.
 *   U = U_s    the "up" case of the same header (s phases of four taps).
 *   adjoint    D^T g = A_H^T g A_W.  The mirror makes it more than a transposed stencil: border pixels also receive the reflected taps.
 *   loss       x [B,C,Hs,Ws] fp32 with strides, y [B,C,H,W] contiguous fp32, Hs = H s, Ws = W s, C 1 or 3, R the data range;
 *              c(t) = clamp(t, 0, R) when the clamp is on and t otherwise;  r = (D c(x) - y) / R (a multiplication by the fp64
 *              reciprocal of R);  rho(r) = |r| for eps = 0 and sqrt(r^2 + eps^2) otherwise;  rho'(r) = sign(r) with sign(0) = 0, or
 *              r / sqrt(r^2 + eps^2);  L = scale * sum rho(r);
 *              dL / dx = scale / R * [0 <= x <= R] * D^T rho'(r)  (the ends of the range pass; the mask only when the clamp is on).
 *   back-projection  r = (y - D c(sr)) / R;  sr <- clamp(fp32(sr + beta R U(r)), 0, R).  The eigenvalues of D U are real and lie in
 *              [0.228, 1] (s = 2, 3, 4, checked numerically per axis up to n = 24 s), so I - beta D U contracts for 0 < beta < 2.
 * Arithmetic: fp64 between the fp32 inputs and the single fp32 rounding of each gradient / updated value; partial sums are folded in
 * a fixed order, no atomics, every output element is written by exactly one thread: two runs are bit-identical, and the result does
 * not depend on the scratch's previous contents.
 * Sizes: H, W >= 1, Hs, Ws <= 16384, B * C <= 65535; anything else is M2T_ERR_ARG before any launch. */
#ifndef M2T_CONSISTENCY_H
#define M2T_CONSISTENCY_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Bytes of device scratch m2t_consistency_loss_tensor / m2t_consistency_loss / m2t_back_project_f32 need for an LR batch [B,C,H,W] at
 * factor `scale`: the fp64 rho' / residual plane (B C H W doubles) and four doubles per tile of 16 x 32 LR cells.  No initialisation
 * needed.  0 for an unsupported shape. */
size_t m2t_consistency_scratch_bytes(int B, int C, int H, int W, int scale);

/* D^T alone: g contiguous [planes,h,w] float32 -> out contiguous [planes,h s,w s]; the fp64 result is rounded once to fp32;
 * accumulate != 0 adds it into out.  M2T_ERR_ARG: a null pointer, scale outside {2, 3, 4}, planes outside 1 .. 65535, h or w < 1, an
 * output side above 16384. */
int m2t_imresize_adjoint_f32(const float* g, int planes, int h, int w, float* out, int scale, int accumulate, void* stream);

/* The plan-free loss (behind losses.consistency_loss / ConsistencyLoss), with the conventions of m2t_gmsd_loss_tensor.  x on the device
 * with image stride x_image_stride, channel stride x_image_stride / C and row stride x_row_stride (elements); y contiguous.
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum rho(r))         (scale = 1 / (B C H W) for the mean)
 *   stats_out   = {mean |r|, max |r|, mean r^2}                                        double[3] on the device, or NULL
 *   gx_add[q]  += (float)(scale / R * (D^T rho'(r))[q])                                x's strides; where clamp != 0 and x[q] is
 *                 outside [0, data_range] the element keeps its bits; elements outside [Hs,Ws] are never touched; NULL = value only
 *                 (no backward launch).
 * scratch: m2t_consistency_scratch_bytes(B, C, H, W, scale_factor) bytes.  M2T_ERR_ARG: a null x / y / loss_out / scratch,
 * scale_factor outside {2, 3, 4}, C other than 1 or 3, B < 1, B * C > 65535, H or W < 1, an SR side above 16384, data_range not a finite
 * number > 0, eps < 0 or not finite, scale not finite, strides that do not hold the image. */
int m2t_consistency_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, int scale_factor, long long x_image_stride,
                                int x_row_stride, float data_range, int clamp, double eps, double scale, float* gx_add, float* loss_out,
                                double* stats_out, int accumulate, void* scratch, void* stream);

/* The same routine on the forward's pre-clamp output (rgb_range = R, the clamp on) against the step's own LR batch lr [B,3,H0,W0],
 * adding into the seed that the immediate pixel loss or the output-gradient setter of m2t.h materialised; exactly 0 in the reflect
 * padding; loss_out as above with scale = weight / divisor.  divisor = the GLOBAL number of LR elements, world * accum * B * 3 * H0 * W0.
 * scratch: m2t_consistency_scratch_bytes(B, 3, H0, W0, plan scale).  State rules of m2t_gmsd_loss: M2T_ERR_STATE without a forward
 * with saved activations, without a seed, or after a deferred pixel loss.  M2T_ERR_ARG: a null argument, a bad rgb_range / divisor /
 * weight, eps < 0 or not finite. */
int m2t_consistency_loss(m2t_plan* p, const float* lr, float weight, double divisor, float rgb_range, double eps, float* loss_out,
                         int accumulate, void* scratch, void* workspace, void* stream);

/* One iteration of back-projection, in place on contiguous sr [B,C,H s,W s] against lr [B,C,H,W]:
 *   r = (lr - D c(sr)) / R in fp64 goes into scratch, c the clamp to [0, data_range];
 *   stats_out (double[3] on the device, or NULL) = {mean |r|, max |r|, mean r^2} of THIS r: the state before the update;
 *   update != 0: sr <- clamp(fp32(sr + beta R U(r)), 0, R); update == 0 computes the statistics only and leaves sr's bits.
 * scratch as above.  M2T_ERR_ARG (before any launch): the list of m2t_consistency_loss_tensor, and beta not finite or outside (0, 2). */
int m2t_back_project_f32(float* sr, const float* lr, int B, int C, int H, int W, int scale_factor, float data_range, double beta,
                         int update, double* stats_out, void* scratch, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
