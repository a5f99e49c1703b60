/* m2t_degrade.h -- LR synthesis beyond bicubic on libm2t.so: a per-sample blur kernel, decimation, speckle and additive noise, in HIP.
 *
 * A thirteenth header on the same library, under the conventions of m2t.h (extern "C", raw device pointers, a hipStream_t passed as
 * void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the twelve older headers are unchanged.
 * Every entry only launches: no allocation, no upload, no host synchronisation, no atomics; they may sit inside a stream capture.
 *
 * What it adds: the reference trains on MATLAB-bicubic pairs only and carries its noise augmentation as dead code
 * (datas/us1k.py:156-167).  This is the classical degradation model  LR = ((HR (*) k) downsampled by s) * (1 + n_s) + n_a  with k and
 * the two levels chosen per sample by the host; the result is defined below to the byte.
 *
 * Definition (scale s in {2, 3, 4}, 3 channels, uint8 HWC images):
 *   bank       M kernels of K x K fp64, row-major [M][K][K], on the device.  K has the parity of s: 1, 3 .. 21 for s = 3; 2, 4 .. 20
 *              for s = 2, 4.  The library does not look at the values (m2trans_amd/degrade.py builds and checks them).
 *   blur       LR pixel (X, Y) in LR-IMAGE coordinates, channel c: first tap column s X + (s - K) / 2, first tap row s Y + (s - K) / 2
 *              (exact integers, possibly negative: the kernel is centred on the pixel's s x s footprint).  A tap outside the image is
 *              folded symmetrically (-1 -> 0, -2 -> 1, N -> N - 1) with period 2N, as often as it takes.
 *              acc = sum_i sum_j w[i][j] * (double)hr[row i][column j][c], rows outer, columns inner, from 0.0, the multiply and the
 *              add rounded separately (no fused multiply-add).
 *   noise      Philox4x32-10, key (seed low word, seed high word), counter (c0, c1, c2, c3): c0 = y * w + x, the pixel's index inside
 *              the item (the patch, or the whole LR image) in source orientation, before the flips; c1 = 3 sel + j + 8 ch with
 *              sel 0 = additive, 1 = speckle, j = 0, 1, 2, ch the channel (0 for every channel when gray); (c2, c3) = low, high word
 *              of noise_id.  With S the integer sum of the twelve words of the blocks j = 0, 1, 2:
 *              g = (2 S + 12 - 12 * 2^32) / 2^33   (Irwin-Hall: unit variance, support +-6, exact in fp64, no transcendental).
 *   value      t = sigma_speckle * g_s;  t = t * acc;  v = acc + t;  u = sigma_add * g_a;  v = v + u;  one rounding per operation;
 *              q = min(max(rint(v), 0), 255), ties to even.  A level of exactly 0 skips its generator and its two operations.
 *              sigma_add is in grey levels (0 .. 255), sigma_speckle is dimensionless.
 *   output     patches: (float)q / 255.f, correctly rounded; whole image: q.
 */
#ifndef M2T_DEGRADE_H
#define M2T_DEGRADE_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Columns of one row of desc_host (long long each). */
#define M2T_DEGRADE_DESC_COLS 11
/*   0  byte offset of the HR image in hr_pool
 *   1  HR image height in pixels          2  HR image row length in pixels
 *   3  lx, 4  ly: the LR corner of the patch (the HR corner is (lx * scale, ly * scale))
 *   5  flags: bit 0 hflip, bit 1 vflip, bit 2 transpose, applied in that order (m2t_crop_patches)
 *   6  bank index                         7  noise_id (all 64 bits)
 *   8  sigma_add, 9  sigma_speckle: the fp64 bit patterns
 *  10  gray: 1 = one variate per pixel shared by the channels, 0 = one per channel */

/* A batch of training pairs cut out of the resident HR pool.  For item i of desc_host [n][M2T_DEGRADE_DESC_COLS] (host memory, read
 * before the call returns; it travels by value in the kernel arguments, 32 items per launch):
 *   lr_out[i] [3][lp][lp] float32, lp = patch_size / scale: the degraded patch as defined above, flipped;
 *   hr_out[i] [3][patch_size][patch_size] float32: bit-identical to m2t_crop_patches.
 * seed is the Philox key.  M2T_ERR_ARG before any launch: a null pointer, n < 1, channels != 3, scale outside {2, 3, 4}, patch_size
 * not a positive multiple of scale, M < 1, K outside its range or of the wrong parity, and per item a negative offset or corner, a
 * patch outside the image, flags > 7, a bank index >= M, a negative or non-finite level, gray outside {0, 1}. */
int m2t_degrade_patches(const unsigned char* hr_pool, const double* bank_dev, int M, int K, const long long* desc_host, int n,
                        int channels, int patch_size, int scale, unsigned long long seed, float* lr_out, float* hr_out, void* stream);

/* A whole image of any aspect ratio: hr_img uint8 [H][W][3] -> lr_u8_out uint8 [H / scale][W / scale][3] (integer division; the taps
 * fold on H and W themselves), the item being the whole LR image.  M2T_ERR_ARG as above, and for H or W below scale. */
int m2t_degrade_image_u8(const unsigned char* hr_img, int H, int W, int channels, const double* bank_dev, int M, int K, int index,
                         int scale, unsigned long long seed, unsigned long long noise_id, double sigma_add, double sigma_speckle,
                         int gray, unsigned char* lr_u8_out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
