/* m2t_resize.h -- the bicubic resampler of libm2t.so: MATLAB-style imresize(..., 'bicubic') by an integer factor 2, 3 or 4, down with
 * antialiasing and up without, in HIP.
 *
 * A third header on the same library, under the conventions of m2t.h and m2t_spectral.h (extern "C", raw device pointers, a
 * hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); m2t.h and
 * m2t_spectral.h are unchanged.  Both entries only launch: no allocation, no upload (the filter taps travel in the kernel
 * arguments), no synchronisation; they may sit inside a stream capture.
 *
 * Definition, per axis of length n, factor s, 0-based indices, k the cubic convolution kernel with a = -0.5
 * (k(x) = 1.5|x|^3 - 2.5|x|^2 + 1 for |x| <= 1, -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 for 1 < |x| <= 2, 0 beyond):
 *   down  n a multiple of s, n / s outputs; output i has centre u = (i + 1/2) s - 1/2 and takes the taps j with |u - j| < 2 s,
 *         weighted k((u - j) / s) / s: one fixed symmetric filter on j = i s + m (8, 9, 16 non-zero taps for s = 2, 3, 4);
 *   up    n s outputs; u = (i + 1/2) / s - 1/2, the four taps j = floor(u) - 1 .. floor(u) + 2 weighted k(u - j): s phases;
 *   both  weights divided by their sum; a tap outside the axis is mirrored with the edge pixel repeated, period 2 n
 *         (j < 0 -> -1 - j, j >= n -> 2 n - 1 - j, applied modulo 2 n: a short axis reflects more than once).
 * Rows (vertical) first, then columns, no rounding between the passes; weights, products and sums in fp64; no atomics: two runs
 * are bit-identical.  For s = 2 and 4 on uint8 data every weight is a multiple of 2^-12, so every product and sum is exact and the
 * rounded result does not depend on the summation order.
 *
 * Parity with MATLAB itself is unpinned: there is no MATLAB and no file of the dataset where this library is built; the definition
 * is pinned by an independent fp64 restatement and by torch's antialiased bicubic interpolation away from the borders. */
#ifndef M2T_RESIZE_H
#define M2T_RESIZE_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* One uint8 image, HWC interleaved: src contiguous [H,W,3] -> dst contiguous [H',W',3], H' = H / scale (up == 0) or H * scale
 * (up != 0), W' likewise; the fp64 result is rounded half away from zero and saturated to [0, 255].
 * Stands in for the offline MATLAB step behind the reference's `_LR_bicubic` folders (datas/us1k.py:84,176: US1K_train_LR_bicubic;
 * datas/benchmark.py: <LR_folder>/X{s}/<name>x{s}): datas.US1K / datas.Benchmark synthesise their LR half with it.
 * M2T_ERR_ARG (before any launch): a null pointer, channels != 3, scale outside {2, 3, 4}, H or W < 1, down with H or W not a
 * multiple of scale, an output side above 16384. */
int m2t_imresize_u8(const unsigned char* src, int H, int W, int channels, unsigned char* dst, int scale, int up, void* stream);

/* float32 planes: src contiguous [planes,H,W] -> dst contiguous [planes,H',W']; the fp64 result is rounded once to fp32, after a
 * clamp to [0, clamp_max] when clamp_max > 0.
 * Stands in for the "Bicubic" row that heads the result tables of the paper (the interpolation baseline the model is scored
 * against; resize.BicubicUp under metrics.evaluate).
 * M2T_ERR_ARG (before any launch): as above, planes outside 1 .. 65535, a clamp_max that is not finite. */
int m2t_imresize_f32(const float* src, int planes, int H, int W, float* dst, int scale, int up, float clamp_max, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
