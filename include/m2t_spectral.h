/* m2t_spectral.h -- the frequency-domain entry points of libm2t.so: a 2-D real FFT in HIP and the L1 loss term on its coefficients.
 *
 * A second header on the same library, under the conventions of m2t.h (extern "C", raw device pointers, a hipStream_t passed as
 * void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); m2t.h itself is unchanged.  The one
 * departure: the table of the N-th roots of unity of a transform length (fp64 on the host, rounded once to fp32, a few KB) is
 * allocated and uploaded by the library ONCE per (calling thread, device, length); the first call with a new H or W therefore
 * synchronises and must not sit inside a stream capture.  Later calls only launch.
 *
 * What it replaces: the reference imports torch.fft (losses.py:5, models/M2Trans_network.py:8) and never calls it; the term is the
 * one MIMO-UNet puts next to its pixel loss, F.l1_loss(view_as_real(rfft2(sr)), view_as_real(rfft2(hr))).
 *
 * Definition, per sample and channel on the H x W image:  x = clamp(pre, 0, R) / R,  y = hr / R,  d = x - y,  D = s * rfft2(d)
 * (H x (W/2+1) complex; s = 1 for norm 0 = "backward", 1 / sqrt(H W) for norm 1 = "ortho"; ONE transform of d, the transform
 * being linear);  loss = weight * mean(|Re D|, |Im D|) over all 2 * B * C * H * (W/2+1) reals.  The imaginary part of the four
 * self-conjugate bins (ky in {0, H/2}, kx in {0, W/2}) is forced to exactly 0 (sign 0; the bins still count in the divisor);
 * sign(0) = 0.  Gradient with respect to pre(h, w):  (weight / divisor) / R * s * Re sum_ky sum_{kx <= W/2} (sign Re D + i sign Im D)
 * e^{+2 pi i (ky h / H + kx w / W)} -- the half spectrum, no Hermitian doubling -- through the clamp mask of the pixel losses (ends
 * of [0, R] included in the pass band).
 *
 * Sizes: H and W even, 8 .. 2048, of the form 2^a * 3^b (every training patch of the shipped configs: 192 .. 768); anything else is
 * M2T_ERR_ARG, decided on the host before any launch.  No Bluestein path, no radix 5 / 7, no odd lengths.
 * Arithmetic: fp32 butterflies (Stockham, radix 4 / 2 / 3, in LDS), fp64 partial sums folded in a fixed order, no atomics: two runs
 * are bit-identical.  Each gradient value is rounded to fp32 once and added in fp32. */
#ifndef M2T_SPECTRAL_H
#define M2T_SPECTRAL_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Bytes of device scratch the two loss entries need for [B,C,H,W] (the fp32 complex half spectrum and one double per workgroup
 * of the column pass; no initialisation needed).  0 for an unsupported size, B or C < 1, or B * C > 65535. */
size_t m2t_fft_loss_scratch_bytes(int B, int C, int H, int W);

/* torch.fft.rfft2(x, norm=...) for x contiguous [planes,H,W] float32 on the device: out [planes,H,W/2+1,2] float32 (real,
 * imaginary).  norm 0 = "backward", 1 = "ortho".  The imaginary part of the self-conjugate bins is exactly 0.  out is also the
 * working storage between the row and the column pass.  M2T_ERR_ARG: a null pointer, planes outside 1 .. 65535, an unsupported
 * size, another norm. */
int m2t_rfft2(const float* x, float* out, int planes, int H, int W, int norm, void* stream);

/* The plan-free loss (behind losses.fft_loss / FFTLoss).  x [B,C,H,W] float32 on the device with image stride x_image_stride,
 * channel stride x_image_stride / C and row stride x_row_stride (elements); y contiguous [B,C,H,W].  With D as above for
 * R = data_range, x clamped to [0, data_range] first when clamp != 0:
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum (|Re D| + |Im D|))     (scale = 1 / reals for the mean)
 *   gx_add[q]  += (float)(scale * d sum / dx[q])      x's strides; where clamp != 0 and x[q] is outside [0, data_range] the element
 *                 is left alone; elements outside [H,W] are never touched; NULL = value only (two launches fewer).
 * scratch: m2t_fft_loss_scratch_bytes(B, C, H, W) bytes.  M2T_ERR_ARG: a null x / y / loss_out / scratch, an unsupported size,
 * data_range not a finite number > 0, another norm, a scale that is not finite, B * C outside 1 .. 65535, strides that do not hold
 * the image. */
int m2t_fft_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                        float data_range, int clamp, int norm, double scale, float* gx_add, float* loss_out, int accumulate,
                        void* scratch, void* stream);

/* The same routine on the forward's pre-clamp output (rgb_range = R, the clamp on), adding into the seed that the immediate pixel
 * loss or the output-gradient setter of m2t.h materialised; exactly 0 in the reflect padding; loss_out as above with
 * scale = weight / divisor.  divisor = the GLOBAL number of reals, world * accum * B * 3 * Hs * (Ws/2+1) * 2, so that rank shards
 * and micro-batches sum to weight * the global mean (the scheme of the pixel term).  scratch: m2t_fft_loss_scratch_bytes(B, 3,
 * Hs, Ws).  State rules of the structural term: M2T_ERR_STATE without a forward with saved activations, without a seed, or after
 * a deferred pixel loss.  M2T_ERR_ARG: a null argument, an SR size that is not supported, a bad rgb_range / divisor / norm. */
int m2t_fft_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, int norm, float* loss_out,
                 int accumulate, void* scratch, void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
