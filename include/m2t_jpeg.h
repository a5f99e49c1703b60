/* m2t_jpeg.h -- JPEG compression artefacts on libm2t.so: a simulated baseline JPEG round trip at 4:4:4 with a per-sample quality, as
 * the last stage of the LR synthesis of m2t_degrade.h or on its own, in HIP.
 *
 * A fourteenth header on the same library, under the conventions of m2t.h (extern "C", raw device pointers, a hipStream_t passed as
 * void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the thirteen older headers are unchanged.
 * The device entries only launch: no allocation, no upload, no host synchronisation, no atomics; they may sit inside a stream
 * capture.
 *
 * What it adds: clinical ultrasound frames reach a super-resolution model as lossy JPEG (DICOM "JPEG baseline", PACS exports, screen
 * captures), and practical degradation pipelines (BSRGAN, Real-ESRGAN) end with a JPEG stage at a random quality.  The stage here is
 * the colour transform, the 8 x 8 DCT, the quantiser of the given quality and the way back; entropy coding is lossless and is not
 * performed.  The result is defined below to the byte.
 *
 * Definition.  Input: the item's lh x lw x 3 8-bit values q in source orientation, before the flips -- for the degrade entries the q
 * of m2t_degrade.h ("value"), for m2t_jpeg_image_u8 any uint8 HWC image.
 *   blocks     8 x 8, anchored at the item's origin (the patch corner, or the whole image's origin).  A block that sticks out of the
 *              item reads q(min(y, lh - 1), min(x, lw - 1)) (libjpeg's edge replication); only pixels inside the item are written.
 *   colour     fp64, one rounding per operation, no fused multiply-add, in the written order:
 *                Y  = rint((0.299 r + 0.587 g) + 0.114 b)
 *                Cb = rint(((128 - 0.168736 r) - 0.331264 g) + 0.5 b)
 *                Cr = rint(((128 + 0.5 r) - 0.418688 g) - 0.081312 b)
 *              each clamped to 0 .. 255, and f = plane - 128.
 *   tables     base: the luminance and chrominance tables of ITU-T T.81 Annex K (the luminance table's first row is
 *              16 11 10 16 24 40 51 61), in natural (row-major) order.  With S = 5000 / quality (integer division) for quality < 50,
 *              else 200 - 2 quality:  Q = min(max((base S + 50) / 100, 1), 255)  (integer division).  Y uses the luminance table,
 *              Cb and Cr the chrominance table.
 *   transform  T[u][x] = c_u cos((2 x + 1) u pi / 16), c_0 = sqrt(1 / 8), c_u = 1 / 2 otherwise.
 *              forward   g[i][v] = sum_j T[v][j] f[i][j];  F[u][v] = sum_i T[u][i] g[i][v]
 *              quantise  c = rint(F * recip[Q[u][v]]), ties to even;  d = c * (double)Q[u][v]
 *              inverse   h[i][v] = sum_u T[u][i] d[u][v];  o[i][j] = sum_v T[v][j] h[i][v];  plane' = min(max(rint(o + 128), 0), 255)
 *              Every sum starts at 0.0, its index ascends, the multiply and the add are separate roundings.
 *   to RGB     cb = Cb' - 128, cr = Cr' - 128:
 *                R = rint(Y' + 1.402 cr);  G = rint((Y' - 0.344136 cb) - 0.714136 cr);  B = rint(Y' + 1.772 cb)
 *              each clamped to 0 .. 255.
 *   constants  consts_dev: M2T_JPEG_CONSTS fp64 values on the device, T[8][8] row-major followed by recip[k] = 1.0 / k, k = 0 .. 255
 *              (recip[0] is unused), built once on the host (m2trans_amd/degrade.py).  The library does not look at the values.  The
 *              device performs no fp64 division and no transcendental.
 *   skip       quality 0 means "stage skipped": the bytes are those of m2t_degrade_patches / m2t_degrade_image_u8.  Otherwise quality
 *              is 1 .. 100.
 *   output     after the stage the flips / transpose and the float32 q / 255 store of m2t_degrade_patches, or the uint8 store.
 *
 * Chroma subsampling (4:2:0) is not built.  For grey frames replicated to RGB, Cb = Cr = 128 exactly, the chroma planes are zero
 * before and after the transform, and every subsampling mode gives the same bytes.  Not built either: a block grid anchored at the
 * frame instead of the patch, second-order degradation, sinc kernels, one-channel images.
 */
#ifndef M2T_JPEG_H
#define M2T_JPEG_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* fp64 values behind consts_dev: T[64], then recip[256]. */
#define M2T_JPEG_CONSTS 320
/* Columns of one row of desc_host of m2t_degrade_jpeg_patches: columns 0 .. 10 as M2T_DEGRADE_DESC_COLS lists them, and
 *  11  quality: 0 = the stage is skipped for this item, 1 .. 100 */
#define M2T_DEGRADE_JPEG_DESC_COLS 12

/* Host only: the two quantisation tables of `quality` (1 .. 100) in natural order, as defined above -- the one definition the
 * kernels share.  M2T_ERR_ARG: a null pointer, quality outside 1 .. 100. */
int m2t_jpeg_quant_tables(int quality, int luma[64], int chroma[64]);

/* The stage alone: img uint8 [H][W][3] -> out uint8 [H][W][3], the item being the whole image (H, W >= 1; out may not overlap img).
 * M2T_ERR_ARG before any launch: a null pointer, channels != 3, H or W < 1 or too large, quality outside 1 .. 100. */
int m2t_jpeg_image_u8(const unsigned char* img, int H, int W, int channels, const double* consts_dev, int quality, unsigned char* out,
                      void* stream);

/* m2t_degrade_patches with the stage between the quantisation and the flips; desc_host is [n][M2T_DEGRADE_JPEG_DESC_COLS].  hr_out is
 * bit-identical to m2t_crop_patches; an item of quality 0 gets the LR bytes of m2t_degrade_patches.  M2T_ERR_ARG before any launch:
 * everything m2t_degrade_patches refuses, a null consts_dev, a quality outside 0 .. 100. */
int m2t_degrade_jpeg_patches(const unsigned char* hr_pool, const double* bank_dev, int M, int K, const double* consts_dev,
                             const long long* desc_host, int n, int channels, int patch_size, int scale, unsigned long long seed,
                             float* lr_out, float* hr_out, void* stream);

/* m2t_degrade_image_u8 with the stage behind it, the item being the whole LR image.  M2T_ERR_ARG before any launch: everything
 * m2t_degrade_image_u8 refuses, a null consts_dev, a quality outside 0 .. 100. */
int m2t_degrade_jpeg_image_u8(const unsigned char* hr_img, int H, int W, int channels, const double* bank_dev, int M, int K, int index,
                              int scale, unsigned long long seed, unsigned long long noise_id, double sigma_add, double sigma_speckle,
                              int gray, const double* consts_dev, int quality, unsigned char* lr_u8_out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
