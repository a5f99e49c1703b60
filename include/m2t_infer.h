/* m2t_infer.h -- the inference end of libm2t.so: the eight flips and transposes of an image as one batch (geometric self-ensemble,
 * the "+" row of an SR results table), their merge into a mean and a per-pixel spread, and the export of a float tensor as an 8-bit
 * image, in HIP.
 *
 * A ninth header on the same library, under the conventions of m2t_resize.h (extern "C", raw device pointers, a hipStream_t passed
 * as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the eight older headers are unchanged.
 * The entries only launch: no allocation, no upload, no synchronisation; they may sit inside a stream capture.  Argument errors are
 * reported before any launch.
 *
 * Views.  One plane x[H,W] and k = 4 t + 2 v + h with t, v, h in {0, 1}:  y[i,j] = x[v ? H-1-i : i, h ? W-1-j : j];
 *   V_k(x) = y for t = 0 (shape [H,W]) and the transpose of y for t = 1 (shape [W,H]).
 * Inverse on an output z_k ([Hs,Ws] for t = 0, [Ws,Hs] for t = 1):  u = z_k for t = 0 and the transpose of z_k for t = 1, then
 *   U_k[i,j] = u[v ? Hs-1-i : i, h ? Ws-1-j : j]  (un-transpose first, then the same flips).
 * Merge, fp32 without contraction:
 *   mean   = (((U0 + U1) + (U2 + U3)) + ((U4 + U5) + (U6 + U7))) * 0.125f
 *   d_k    = U_k - mean
 *   var    = (((d0 d0 + d1 d1) + (d2 d2 + d3 d3)) + ((d4 d4 + d5 d5) + (d6 d6 + d7 d7))) * 0.125f
 *   spread = sqrtf(var)
 * Export (the rounding of torchvision's save_image):  dst[i,j,c] = (uint8) min(max(src[c,i,j] * s + 0.5f, 0.f), 255.f), the cast
 *   truncating, s = 255.0f / rgb_range formed once on the host in fp32; a NaN becomes 0.
 * No atomics: two runs are bit-identical. */
#ifndef M2T_INFER_H
#define M2T_INFER_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* src contiguous [planes,H,W] -> dst_a contiguous [4,planes,H,W] (views k = 0 .. 3) and dst_b contiguous [4,planes,W,H] (views
 * k = 4 .. 7).  With planes = 3 B the destinations are the batches [4B,3,H,W] and [4B,3,W,H]: view k of image b sits at batch index
 * (k mod 4) B + b.  For H == W the caller may place dst_b directly behind dst_a and treat both as one [8B,3,H,H] batch.
 * M2T_ERR_ARG (before any launch): a null pointer, planes outside 1 .. 65535, H or W outside 1 .. 16384. */
int m2t_dihedral_pack(const float* src, int planes, int H, int W, float* dst_a, float* dst_b, void* stream);

/* sr_a contiguous [4,planes,Hs,Ws] (the outputs of views 0 .. 3), sr_b contiguous [4,planes,Ws,Hs] (views 4 .. 7) -> mean and
 * spread contiguous [planes,Hs,Ws].  spread may be null: then no spread is formed or written.
 * M2T_ERR_ARG (before any launch): a null sr_a / sr_b / mean, planes outside 1 .. 65535, Hs or Ws outside 1 .. 16384. */
int m2t_dihedral_merge(const float* sr_a, const float* sr_b, int planes, int Hs, int Ws, float* mean, float* spread, void* stream);

/* src contiguous float32 [channels,H,W] -> dst contiguous uint8 [H,W,channels], channels 1 or 3.
 * M2T_ERR_ARG (before any launch): a null pointer, channels outside {1, 3}, H or W outside 1 .. 16384, an rgb_range that is not a
 * finite number > 0. */
int m2t_tensor_to_image_u8(const float* src, int channels, int H, int W, float rgb_range, unsigned char* dst, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
