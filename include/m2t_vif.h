/* m2t_vif.h -- the information-fidelity loss term of libm2t.so: 1 - VIF (pixel domain) with its gradient, in HIP.
 *
 * A fifth header on the same library, under the conventions of m2t.h, m2t_spectral.h, m2t_resize.h and m2t_msssim.h (extern "C", raw
 * device pointers, a hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the
 * four older headers are unchanged.  Every entry only launches: no allocation, no upload, no host synchronisation; they may sit
 * inside a stream capture.
 *
 * What it replaces: the reference imports VIFLoss from piq next to the pixel criteria (losses.py:8); pixel-domain VIF (Sheikh &
 * Bovik, "Image information and visual quality"; piq.vif_p) is also a score of ultrasound-SR tables.
 *
 * Definition, per image b; R = data range, EPS = 1e-8, n = sigma_n_sq (2.0 by default); everything after the fp32 inputs is fp64:
 *   luminance  u_0 = (255 / R) * (0.299 c(x_R) + 0.587 c(x_G) + 0.114 c(x_B)), c(t) = clamp(t, 0, R) when the clamp is on and t
 *              otherwise; v_0 the same of y, never clamped; with one channel u_0 = 255 / R * c(x).  C is 1 or 3.
 *   scales     s = 0 .. 3, window length N_s = 2^(4 - s) + 1 (17, 9, 5, 3), taps g_s[k] = exp(-(k - (N_s - 1) / 2)^2 / (2 (N_s / 5)^2))
 *              normalised to sum 1, evaluated in fp64, applied separably, VALID.
 *   pyramid    for s > 0: u_s = (G_s * u_{s-1})[::2, ::2] (a VALID filter with this scale's window, then every second row and
 *              column from 0); v_s likewise.
 *   moments    under G_s, VALID: mx = G*u, my = G*v, a = max(G*(u u) - mx^2, 0), b = max(G*(v v) - my^2, 0), c = G*(u v) - mx my.
 *   map        live = b >= EPS and a >= EPS and c >= 0;  g = c / (b + EPS);  sv_raw = a - g c;  sv = sv_raw if sv_raw > EPS else EPS;
 *              t = log10(1 + g^2 b / (sv + n)) where live, exactly 0 elsewhere;  d = log10(1 + b / n) where b >= EPS, 0 elsewhere.
 *   score      VIF_b = (sum_s sum_map t + EPS) / (sum_s sum_map d + EPS);   term = weight * (1 - mean_b VIF_b).
 * VIF exceeds 1 for a contrast-enhanced x, so the term may be NEGATIVE; it is not clipped.
 * Gradient, with respect to x only (the denominator depends on y alone).  Where live, with q = g^2 b, z = sv + n,
 * k = 1 / (ln 10 (1 + q / z)):  dt/da = -k q / z^2 if sv_raw > EPS else 0;
 * dt/dc = k (2 c b / ((b + EPS)^2 z) + (q / z^2) (2 c / (b + EPS) if sv_raw > EPS else 0));  both exactly 0 where not live.
 * d sum(t_s) / du_s(p) = 2 u(p) G^T[dt/da](p) + v(p) G^T[dt/dc](p) + G^T[-2 mx dt/da - my dt/dc](p); the gradient with respect to u_s
 * is that plus the adjoint of (filter, decimate) applied to the gradient with respect to u_{s+1} (zero-stuffing by 2, then the
 * transposed G_{s+1}), from the coarsest scale to the finest;  dVIF_b / du_0 = (d sum t / du_0) / (sum d + EPS);  to channel ch with
 * luminance weight w_ch: times w_ch * 255 / R * [0 <= x_ch <= R] (the ends of the range pass; the mask only when the clamp is on).
 * An image whose y is flat under every window has VIF = 1 and gradient exactly 0.
 *
 * Sizes: min(H, W) >= 41 (at 41 the scale-3 map is 1 x 1; the packages' own minimum); anything smaller is M2T_ERR_ARG before any
 * launch.  B <= 65535.  Arithmetic: fp64 between the fp32 inputs and the one fp32 rounding of each gradient value; partial sums are
 * folded in a fixed order, no atomics, every output element is written by exactly one thread: two runs are bit-identical.
 * Parity with piq itself is unpinned (it is not installed where this library is built); the definition is pinned by an fp64
 * restatement and torch autograd. */
#ifndef M2T_VIF_H
#define M2T_VIF_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Bytes of device scratch the two loss entries need for [B,C,H,W]: the per-image record, the partial sums, levels 1 .. 3 of both
 * fp64 pyramids and the fp64 gradient levels 1 .. 3.  No initialisation needed.  0 for min(H, W) < 41, C other than 1 or 3, B < 1
 * or B > 65535. */
size_t m2t_vif_loss_scratch_bytes(int B, int C, int H, int W);

/* Where a region of that scratch starts (bytes), for audits and tests; (size_t)-1 for an unsupported shape, region or level.
 *   region 0: the record, 4 doubles per image: sum t, sum d, VIF_b, scale / (sum d + EPS)
 *   region 1: the partial sums of scale `level` (0 .. 3), [B][tiles][2] (t, d), tiles of 16 x 16 pixels of that level
 *   region 2 / 3: level `level` (1 .. 3) of the u / v pyramid, contiguous [B][H_s][W_s] doubles
 *   region 4: the gradient of sum t with respect to level `level` (1 .. 3), the same shape (written only with gx_add != NULL) */
size_t m2t_vif_loss_scratch_offset(int B, int C, int H, int W, int region, int level);

/* The plan-free loss (behind losses.vif_loss / VIFLoss and metrics.vif_device).  x [B,C,H,W] float32 on the device with image stride
 * x_image_stride, channel stride x_image_stride / C and row stride x_row_stride (elements); y contiguous [B,C,H,W].  With VIF_b as
 * above for R = data_range and n = sigma_n_sq, x clamped to [0, data_range] first when clamp != 0:
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum_b (1 - VIF_b))           (scale = 1 / B for the mean)
 *   per_image_out[b] = VIF_b                                                double[B] on the device, or NULL
 *   gx_add[q]  += (float)(-scale * dVIF_b / dx[q])                          x's strides; where clamp != 0 and x[q] is outside
 *                 [0, data_range] the element is left alone; elements outside [H,W] are never touched; NULL = value only (no
 *                 gradient launches).
 * scratch: m2t_vif_loss_scratch_bytes(B, C, H, W) bytes.  M2T_ERR_ARG: a null x / y / loss_out / scratch, B outside 1 .. 65535,
 * C other than 1 or 3, min(H, W) < 41, data_range or sigma_n_sq not a finite number > 0, strides that do not hold the image. */
int m2t_vif_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                        float data_range, double sigma_n_sq, int clamp, double scale, float* gx_add, float* loss_out,
                        double* per_image_out, int accumulate, void* scratch, void* stream);

/* The same routine on the forward's pre-clamp output (rgb_range = R, the clamp on), adding into the seed that the immediate pixel
 * loss or the output-gradient setter of m2t.h materialised; exactly 0 in the reflect padding; loss_out as above with
 * scale = weight / divisor.  divisor = the GLOBAL number of images, world * accum * B (not times 3: the luminance collapses the
 * channels), so that rank shards and micro-batches sum to weight * (1 - the global mean VIF).  scratch:
 * m2t_vif_loss_scratch_bytes(B, 3, Hs, Ws).  State rules of m2t_ssim_loss: M2T_ERR_STATE without a forward with saved activations,
 * without a seed, or after a deferred pixel loss.  M2T_ERR_ARG: a null argument, an SR side < 41, a bad rgb_range / divisor /
 * weight / sigma_n_sq. */
int m2t_vif_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, double sigma_n_sq, float* loss_out,
                 int accumulate, void* scratch, void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
