/* m2t_train.h -- the training-loop end of libm2t.so: a device-resident meter for the per-step loss values (so that the epoch loop
 * logs without a host synchronisation per step) and the "LR upsampled | SR | HR" preview strip of one sample as an 8-bit image, in
 * HIP.
 *
 * A tenth header on the same library, under the conventions of m2t_infer.h (extern "C", raw device pointers, a hipStream_t passed
 * as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the nine older headers are unchanged.
 * The entries only launch: no allocation, no upload, no synchronisation; they may sit inside a stream capture.  Argument errors are
 * decided on the host before any launch.  No atomics and no scratch: two runs are bit-identical.
 *
 * Meter.  `record` holds 8 doubles per column c, at record[8 c + k]:
 *   k = 0 sum of the finite samples (fp64, in call order: equal, bit for bit, to a sequential fp64 sum on the host)
 *   k = 1 number of finite samples          k = 2 number of non-finite samples
 *   k = 3 minimum of the finite samples     k = 4 maximum of the finite samples     k = 5 the last sample, finite or not
 *   k = 6, 7 reserved (reset writes 0, update leaves them alone)
 * A non-finite sample bumps k = 2 and sets k = 5; it leaves sum, minimum and maximum alone.  Minimum and maximum are updated as
 * `v < min ? v : min` and `v > max ? v : max`.
 * `ring` is float32 [ring_rows, n_cols + 1]: row (step mod ring_rows) receives (float) step and the samples rounded to fp32 (round
 * to nearest even); the column of an absent sample receives a quiet NaN.
 *
 * Preview.  q(v) = trunc(min(max((255.0f * v) / rgb_range, 0), 255)) in fp32 with IEEE division, a NaN becomes 0 (the quantisation
 * of the reference's ldr_f2u, made total: truncation, not the rounding of m2t_infer.h's export).  dst is uint8 [h s, 3 w s, 3]:
 * columns [0, w s) the upsampled LR, [w s, 2 w s) SR, [2 w s, 3 w s) HR.  The LR third is bilinear on the QUANTISED values with
 * half-pixel centres and clamped borders, in integers: along one axis, destination index i has n = 2 i + 1 - s, i0 = floor(n / 2s),
 * f = n - 2s i0, the taps clamp(i0) and clamp(i0 + 1) with the weights 2s - f and f; a pixel is
 *   (sum over the four taps of wy wx q + 2 s^2) / (4 s^2), the division truncating. */
#ifndef M2T_TRAIN_H
#define M2T_TRAIN_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define M2T_METER_MAX_COLS 16
#define M2T_METER_RECORD_DOUBLES 8

/* record [n_cols * 8] doubles: sum 0, counts 0, minimum +inf, maximum -inf, last 0, reserved 0; ring [ring_rows, n_cols + 1]
 * floats: NaN.  One launch.
 * M2T_ERR_ARG (before any launch): a null record or ring, n_cols outside 1 .. 16, ring_rows outside 1 .. 2^24. */
int m2t_meter_reset(double* record, float* ring, int n_cols, int ring_rows, void* stream);

/* values and kinds are HOST arrays of n_cols entries.  values[c] is a DEVICE pointer to one scalar, float32 for kinds[c] = 0 and
 * float64 for kinds[c] = 1; a null values[c] marks a column that is absent this step: its record is not touched.  The pointers
 * travel to the kernel by value in its argument block: there is no host-to-device copy, and the host arrays may be freed on
 * return.  One launch of one wavefront, thread c owns column c.
 * M2T_ERR_ARG (before any launch): a null values / kinds / record / ring, n_cols outside 1 .. 16, ring_rows outside 1 .. 2^24, a
 * kind outside {0, 1}, a negative step. */
int m2t_meter_update(const void* const* values, const int* kinds, int n_cols, double* record, float* ring, int ring_rows, long long step, void* stream);

/* lr contiguous float32 [3,h,w], sr and hr contiguous float32 [3,h*scale,w*scale] -> dst contiguous uint8 [h*scale, 3*w*scale, 3].
 * M2T_ERR_ARG (before any launch): a null pointer, a scale outside {2, 3, 4}, h or w < 1, h*scale or w*scale above 16384, an
 * rgb_range that is not a finite number > 0. */
int m2t_preview_strip(const float* lr, const float* sr, const float* hr, int h, int w, int scale, float rgb_range, unsigned char* dst, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
