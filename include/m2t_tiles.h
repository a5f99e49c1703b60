/* m2t_tiles.h -- tiled inference on libm2t.so: an image is cut into overlapping tiles of the training size, the model runs on the
 * tiles as batches, and the outputs are feather-blended into one image, in HIP.  Every CFTM block of the model normalises over the
 * plane it is given (an InstanceNorm without affine part or running statistics), so tiles of the training size give it the statistics
 * it was trained with; and every image of every size runs on one (tile_batch, T, T) plan.
 *
 * An eleventh header on the same library, under the conventions of m2t_infer.h (extern "C", raw device pointers, a hipStream_t passed
 * as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the ten older headers are unchanged.
 * The device entries only launch: no allocation, no upload, no synchronisation; they may sit inside a stream capture.  Argument
 * errors are decided on the host before any launch.  No atomics and no scratch: two runs are bit-identical.
 *
 * Grid.  One axis of LR length L, tile size T >= 1, overlap v with 0 <= 2 v <= T:
 *   L <= T:    one tile, n = 1, length t = L, origin 0;
 *   otherwise  t = T, S = T - v, n = ceil((L - T) / S) + 1, o_k = min(k S, L - T): every tile lies inside the image, the last one is
 *              shifted back.  The origins increase strictly, every pixel is covered, and no pixel by more than 3 tiles (2 v <= T
 *              keeps regular tiles two apart from overlapping; the third is the shifted last tile).
 * All tiles of an image have the shape th x tw (the two axes' t).  Tile (b, ky, kx) of a batch [B, ...] has the global index
 *   g = (b ny + ky) nx + kx.
 *
 * Blend.  SR pixel units, scale s, fp64, every operation a single IEEE operation (no contraction).  On one axis tile k covers the
 * SR coordinates p with u = p - s o_k in [0, s t):
 *   a_k = s (o_{k-1} + t - o_k) for k >= 1, else 0       (the overlap with the previous tile)
 *   b_k = s (o_k + t - o_{k+1}) for k <= n - 2, else 0   (the overlap with the next tile)
 *   w_k(u) = min(1, a_k > 0 ? (u + 0.5) / a_k : 1, b_k > 0 ? (s t - u - 0.5) / b_k : 1)       (positive on the whole tile)
 * and Wt = wy * wx in 2-D.  Per output element, over the covering tiles, ky ascending outside and kx ascending inside, each sum
 * starting at 0.0 and growing by one addition per tile:
 *   num = sum Wt * (double) z,   den = sum Wt,   m = num / den,   out = (float) m
 *   seam = sqrtf((float) (q / den)),   q = sum Wt * (d * d),   d = (double) z - m        (how much the tiles disagree where they meet)
 * An element covered by exactly one tile is copied: out = z, seam = 0. */
#ifndef M2T_TILES_H
#define M2T_TILES_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Host only, no device involved: the grid of one axis.  *n_out = the number of tiles, *tile_len_out = t, origins_out[0 .. n-1] = o_k
 * (may be NULL: call once for n, then again with n ints).
 * M2T_ERR_ARG: a null n_out or tile_len_out, L or T outside 1 .. 16384, overlap < 0 or 2 overlap > T. */
int m2t_tile_grid(int L, int T, int overlap, int* n_out, int* tile_len_out, int* origins_out /* n ints, may be NULL */);

/* src contiguous [B,C,H,W] -> dst contiguous [count,C,th,tw]: the tiles first .. first + count - 1 of the global order.
 * M2T_ERR_ARG (before any launch): a null pointer, H, W or T outside 1 .. 16384, overlap < 0 or 2 overlap > T, B C outside
 * 1 .. 65535 (B, C >= 1), first < 0, count < 1, first + count above the tile count B ny nx, count C above 2^22. */
int m2t_tile_gather(const float* src, int B, int C, int H, int W, int T, int overlap, int first, int count, float* dst, void* stream);

/* tiles contiguous [B ny nx, C, s th, s tw] (the outputs of the tiles, global order) -> dst contiguous [B,C,s H,s W] and, unless
 * null, seam of the same shape.  With a null seam nothing of it is formed or written.
 * M2T_ERR_ARG (before any launch): a null tiles or dst, H, W or T outside 1 .. 16384, overlap < 0 or 2 overlap > T, scale outside
 * 1 .. 8, s H or s W above 65536, B C outside 1 .. 65535 (B, C >= 1). */
int m2t_tile_blend(const float* tiles, int B, int C, int H, int W, int T, int overlap, int scale, float* dst, float* seam /* may be NULL */, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
