// k_train.hip -- the training-loop end (include/m2t_train.h): the step meter that keeps the per-step loss values of the epoch loop on
// the device (the reference reads them with three float(loss) per step, train.py:212-214: three host synchronisations), and the
// "LR upsampled | SR | HR" preview strip of one sample (train.py:219-231 builds it on the host with numpy and cv2).
//
// Meter: one wavefront, thread c owns column c of the record and of the ring row; the device pointers of the samples arrive by
// value in the kernel's argument block (kernarg segment), so the host uploads nothing.  A column is touched by one thread only and
// the sum is a plain fp64 add per call: call order is summation order.
//
// Preview: a workgroup (256 threads = 8 rows of 32 lanes) owns one 32 x 32 tile of output pixels of one third of the strip.  Lane
// tx walks the fastest axis of the planes it reads.  The interleaved destination row of a tile is 96 consecutive bytes, which is
// 24 dwords: the quantised values are staged through LDS PLANAR, one dword per value, [3][32] rows at a pitch of 33 dwords, and the
// 3-byte pixels are put together in registers on the way out.  ds_write_b32 / ds_read_b32 are banked over 32 dwords in the two
// 32-lane halves of a wave; a half is one tile row here in both phases.  The fill puts lane tx at dword (32 c + r) * 33 + tx, bank
// (r + tx) mod 32; the drain has lane d (d < 24: one output dword) read, for each of its four bytes k, pixel (4 d + k) / 3 of plane
// (4 d + k) mod 3: for a fixed k the 24 pixels are distinct, so are the banks (r + pixel) mod 32 -- no conflict either way, and none
// of the 2-way / 4-way conflicts that byte writes at a pitch of 3 bytes (four lanes to a dword) would bring.  Lanes 24 .. 31 idle
// in the drain.  A row whose destination is not dword aligned, or that an edge tile cuts short, is stored byte by byte by the same
// lanes (still consecutive addresses).  Edge tiles are predicated per element, offsets are 64-bit, no atomics, no scratch.
#include "m2t_common.h"
#include "../../include/m2t_train.h"
#include <math.h>

namespace {

constexpr int TILE = 32;
constexpr int PITCH = TILE + 1;
constexpr int RPT = TILE / 8;                  // tile rows per thread
constexpr int MAX_SIDE = 16384;
constexpr int MAX_RING_ROWS = 1 << 24;
constexpr int REC = M2T_METER_RECORD_DOUBLES;

struct MeterArgs {
  const void* values[M2T_METER_MAX_COLS];
  int kinds[M2T_METER_MAX_COLS];
  double* record;
  float* ring;
  long long step;
  int n_cols, ring_rows;
};

__global__ __launch_bounds__(256) void meter_reset_kernel(double* __restrict__ record, float* __restrict__ ring, int n_cols, long long n_ring) {
  const int t = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  for (int i = t; i < n_cols * REC; i += stride) {
    const int k = i % REC;
    record[i] = k == 3 ? (double)INFINITY : k == 4 ? -(double)INFINITY : 0.0;
  }
  for (long long i = t; i < n_ring; i += stride) ring[i] = __builtin_nanf("");
}

__global__ __launch_bounds__(M2T_WAVE) void meter_update_kernel(const MeterArgs a) {
  const int c = threadIdx.x;
  if (c >= a.n_cols) return;
  float* row = a.ring + (a.step % a.ring_rows) * (long long)(a.n_cols + 1);
  if (c == 0) row[0] = (float)a.step;
  const void* p = a.values[c];
  if (!p) {
    row[c + 1] = __builtin_nanf("");
    return;
  }
  const double v = a.kinds[c] ? *static_cast<const double*>(p) : (double)*static_cast<const float*>(p);
  double* r = a.record + (long long)c * REC;
  if (isfinite(v)) {
    r[0] += v;
    r[1] += 1.0;
    const double lo = r[3], hi = r[4];
    r[3] = v < lo ? v : lo;
    r[4] = v > hi ? v : hi;
  } else {
    r[2] += 1.0;
  }
  r[5] = v;
  row[c + 1] = (float)v;
}

// trunc(min(max((255 v) / range, 0), 255)); the comparisons send a NaN to 0
__device__ __forceinline__ uint32_t quantise(float v, float range) {
  float t = (255.0f * v) / range;
  t = t > 0.f ? t : 0.f;
  t = t < 255.f ? t : 255.f;
  return (uint32_t)(int)t;
}

// destination index i of one axis at scale s -> the two clamped taps and the weight f of the second one (out of 2 s)
__device__ __forceinline__ void taps(int i, int s, int n, int& t0, int& t1, int& f) {
  const int num = 2 * i + 1 - s;                       // >= 1 - s
  const int i0 = (num + 2 * s) / (2 * s) - 1;          // floor(num / 2s) for num >= -2s
  f = num - 2 * s * i0;
  t0 = i0 < 0 ? 0 : (i0 > n - 1 ? n - 1 : i0);
  t1 = i0 + 1 > n - 1 ? n - 1 : i0 + 1;                // (i0 + 1 >= 0 always)
}

// grid (tiles along Ws, tiles along Hs, 3 thirds of the strip)
__global__ __launch_bounds__(256) void preview_strip_kernel(const float* __restrict__ lr, const float* __restrict__ sr,
                                                            const float* __restrict__ hr, int h, int w, int s, float range,
                                                            uint8_t* __restrict__ dst) {
  __shared__ uint32_t tile[3 * TILE * PITCH];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE, third = blockIdx.z;
  const int Hs = h * s, Ws = w * s;
  const long long hw = (long long)h * w, HW = (long long)Hs * Ws;

  if (third == 0) {
    const int den = 4 * s * s;
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int r = ty + 8 * q, i = i0 + r, j = j0 + tx;
      if (i < Hs && j < Ws) {
        int y0, y1, fy, x0, x1, fx;
        taps(i, s, h, y0, y1, fy);
        taps(j, s, w, x0, x1, fx);
        const int wy0 = 2 * s - fy, wx0 = 2 * s - fx;
        const long long a = (long long)y0 * w, b = (long long)y1 * w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* p = lr + c * hw;
          const int acc = wy0 * (wx0 * (int)quantise(p[a + x0], range) + fx * (int)quantise(p[a + x1], range)) +
                          fy * (wx0 * (int)quantise(p[b + x0], range) + fx * (int)quantise(p[b + x1], range));
          tile[(c * TILE + r) * PITCH + tx] = (uint32_t)((acc + den / 2) / den);
        }
      }
    }
  } else {
    const float* src = third == 1 ? sr : hr;
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int r = ty + 8 * q, i = i0 + r, j = j0 + tx;
      if (i < Hs && j < Ws) {
        const long long o = (long long)i * Ws + j;
#pragma unroll
        for (int c = 0; c < 3; ++c) tile[(c * TILE + r) * PITCH + tx] = quantise(src[c * HW + o], range);
      }
    }
  }
  __syncthreads();
  // ---- drain: row r of the tile is the bytes [0, 3 * cols) behind dst + ((i * 3 Ws) + third * Ws + j0) * 3
  const int cols = Ws - j0 < TILE ? Ws - j0 : TILE;
  if (tx < 3 * TILE / 4) {
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int r = ty + 8 * q, i = i0 + r;
      if (i >= Hs) continue;
      uint8_t* out = dst + ((long long)i * 3 * Ws + (long long)third * Ws + j0) * 3;
      uint32_t bytes[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = 4 * tx + k, px = e / 3, c = e - 3 * px;
        bytes[k] = px < cols ? tile[(c * TILE + r) * PITCH + px] : 0u;
      }
      if (cols == TILE && ((uintptr_t)out & 3) == 0) {
        reinterpret_cast<uint32_t*>(out)[tx] = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * tx + k < 3 * cols) out[4 * tx + k] = (uint8_t)bytes[k];
      }
    }
  }
}

const char* meter_args(const void* record, const void* ring, int n_cols, int ring_rows) {
  if (!record || !ring) return "null pointer";
  if (n_cols < 1 || n_cols > M2T_METER_MAX_COLS) return "n_cols must be 1 .. 16";
  if (ring_rows < 1 || ring_rows > MAX_RING_ROWS) return "ring_rows must be 1 .. 2^24";
  return nullptr;
}

}  // namespace

extern "C" int m2t_meter_reset(double* record, float* ring, int n_cols, int ring_rows, void* stream) {
  if (const char* bad = meter_args(record, ring, n_cols, ring_rows)) return m2t_set_error_at(M2T_ERR_ARG, "m2t_meter_reset", bad);
  const long long n_ring = (long long)ring_rows * (n_cols + 1);
  const long long blocks = ceil_divll(n_ring, 256);
  meter_reset_kernel<<<(int)(blocks < 1024 ? blocks : 1024), 256, 0, (hipStream_t)stream>>>(record, ring, n_cols, n_ring);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" int m2t_meter_update(const void* const* values, const int* kinds, int n_cols, double* record, float* ring, int ring_rows,
                                long long step, void* stream) {
  const char* bad = meter_args(record, ring, n_cols, ring_rows);
  if (!bad && (!values || !kinds)) bad = "null pointer";
  if (!bad && step < 0) bad = "step must be >= 0";
  MeterArgs a = {};
  if (!bad) {
    for (int c = 0; c < n_cols; ++c) {
      if (kinds[c] != 0 && kinds[c] != 1) {
        bad = "a kind must be 0 (float32) or 1 (float64)";
        break;
      }
      a.values[c] = values[c];
      a.kinds[c] = kinds[c];
    }
  }
  if (bad) return m2t_set_error_at(M2T_ERR_ARG, "m2t_meter_update", bad);
  a.record = record;
  a.ring = ring;
  a.step = step;
  a.n_cols = n_cols;
  a.ring_rows = ring_rows;
  meter_update_kernel<<<1, M2T_WAVE, 0, (hipStream_t)stream>>>(a);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" int m2t_preview_strip(const float* lr, const float* sr, const float* hr, int h, int w, int scale, float rgb_range,
                                 unsigned char* dst, void* stream) {
  const char* bad = nullptr;
  if (!lr || !sr || !hr || !dst) bad = "null pointer";
  else if (scale < 2 || scale > 4) bad = "scale must be 2, 3 or 4";
  else if (h < 1 || w < 1) bad = "h and w must be >= 1";
  else if (h > MAX_SIDE / scale || w > MAX_SIDE / scale) bad = "h * scale and w * scale must be <= 16384";
  else if (!isfinite(rgb_range) || !(rgb_range > 0.f)) bad = "rgb_range must be a finite number > 0";
  if (bad) return m2t_set_error_at(M2T_ERR_ARG, "m2t_preview_strip", bad);
  const dim3 grid(ceil_div(w * scale, TILE), ceil_div(h * scale, TILE), 3);
  preview_strip_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(lr, sr, hr, h, w, scale, rgb_range, dst);
  M2T_LAUNCH_CHECK();
  return 0;
}
