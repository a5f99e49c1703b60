// k_infer.hip -- the inference end (include/m2t_infer.h): the eight dihedral views of a plane (geometric self-ensemble), the merge of
// the eight outputs into a mean and a per-pixel spread, and the export of a float tensor as an 8-bit interleaved image (the rounding
// of torchvision's save_image; the reference's test.py / train.py:275-278 write their results with it).
//
// Pure data movement, so the one thing to get right is that every global load and store runs along the fastest axis.  A workgroup
// (256 threads = 8 rows of 32 lanes) owns one 32 x 32 tile of the un-transposed plane; lane tx always walks the fastest axis of the
// tensor it touches (backwards for a horizontal flip: the same 128-byte segments).
//   pack   reads its source tile once, row-wise: the four un-transposed views are stored straight from the registers; the tile also
//          goes to LDS and the four transposed views are stored from its columns.
//   merge  reads the four tiles of sr_a row-wise into registers and the four of sr_b row-wise (rows of the TRANSPOSED tensor) into
//          LDS, picks those up column-wise, keeps the eight values of a pixel in registers for mean and spread, stores one or two
//          rows.
// LDS tile: 32 rows at a pitch of 33 dwords.  ds_write_b32 / ds_read_b32 are banked over 32 dwords in the two 32-lane halves of a
// wave; a half is one tile row.  The row-wise fill puts lane tx at dword r * 33 + tx (bank (r + tx) mod 32), the column-wise read at
// tx * 33 + r (bank (tx + r) mod 32): 32 distinct banks either way, no conflict.
// Edge tiles are predicated per element, offsets are 64-bit, no atomics (two runs are bit-identical), no scratch.
#include "m2t_common.h"
#include "../../include/m2t_infer.h"
#include <math.h>

namespace {

constexpr int TILE = 32;
constexpr int PITCH = TILE + 1;
constexpr int RPT = TILE / 8;                  // tile rows per thread
constexpr int MAX_SIDE = 16384, MAX_PLANES = 65535;

// grid (tiles along W, tiles along H, planes)
__global__ __launch_bounds__(256) void dihedral_pack_kernel(const float* __restrict__ src, int planes, int H, int W,
                                                            float* __restrict__ dst_a, float* __restrict__ dst_b) {
  __shared__ float tile[TILE * PITCH];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
  const long long hw = (long long)H * W, pl = blockIdx.z;
  const float* x = src + pl * hw;
  float* a = dst_a + pl * hw;                  // view k of this plane: + k * planes * hw
  float* b = dst_b + pl * hw;
  const long long vs = (long long)planes * hw;

  // ---- views 0 .. 3 from the registers: source (si, sj) -> (v ? H-1-si : si, h ? W-1-sj : sj), lanes along sj
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int r = ty + 8 * q, si = i0 + r, sj = j0 + tx;
    if (si < H && sj < W) {
      const float v = x[(long long)si * W + sj];
      tile[r * PITCH + tx] = v;
      const long long row = (long long)si * W, frow = (long long)(H - 1 - si) * W;
      const int fj = W - 1 - sj;
      a[row + sj] = v;
      a[vs + row + fj] = v;
      a[2 * vs + frow + sj] = v;
      a[3 * vs + frow + fj] = v;
    }
  }
  __syncthreads();
  // ---- views 4 .. 7 from the columns of the tile: source (si, sj) -> row (h ? W-1-sj : sj), column (v ? H-1-si : si) of a [W,H]
  // plane, lanes along si
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int r = ty + 8 * q, si = i0 + tx, sj = j0 + r;
    if (si < H && sj < W) {
      const float v = tile[tx * PITCH + r];
      const long long row = (long long)sj * H, frow = (long long)(W - 1 - sj) * H;
      const int fi = H - 1 - si;
      b[row + si] = v;
      b[vs + frow + si] = v;
      b[2 * vs + row + fi] = v;
      b[3 * vs + frow + fi] = v;
    }
  }
}

// grid (tiles along Ws, tiles along Hs, planes)
template <bool SPREAD>
__global__ __launch_bounds__(256) void dihedral_merge_kernel(const float* __restrict__ sr_a, const float* __restrict__ sr_b, int planes,
                                                             int Hs, int Ws, float* __restrict__ mean, float* __restrict__ spread) {
  __shared__ float tile[4][TILE * PITCH];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
  const long long hw = (long long)Hs * Ws, pl = blockIdx.z;
  const float* a = sr_a + pl * hw;
  const float* b = sr_b + pl * hw;
  const long long vs = (long long)planes * hw;

  // ---- U0 .. U3 of pixel (i, j) = sr_a[k][v ? Hs-1-i : i, h ? Ws-1-j : j], lanes along j: issued first, in flight across the barrier
  float u[RPT][8];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int i = i0 + ty + 8 * q, j = j0 + tx;
    if (i < Hs && j < Ws) {
      const long long row = (long long)i * Ws, frow = (long long)(Hs - 1 - i) * Ws;
      const int fj = Ws - 1 - j;
      u[q][0] = a[row + j];
      u[q][1] = a[vs + row + fj];
      u[q][2] = a[2 * vs + frow + j];
      u[q][3] = a[3 * vs + frow + fj];
    }
  }
  // ---- U4 .. U7 of pixel (i, j) = z_k[h ? Ws-1-j : j, v ? Hs-1-i : i] with z_k = sr_b[k - 4] of shape [Ws,Hs]: lanes along i into
  // tile[k - 4][j - j0][i - i0]
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int r = ty + 8 * q, i = i0 + tx, j = j0 + r;
    if (i < Hs && j < Ws) {
      const long long row = (long long)j * Hs, frow = (long long)(Ws - 1 - j) * Hs;
      const int fi = Hs - 1 - i;
      tile[0][r * PITCH + tx] = b[row + i];
      tile[1][r * PITCH + tx] = b[vs + frow + i];
      tile[2][r * PITCH + tx] = b[2 * vs + row + fi];
      tile[3][r * PITCH + tx] = b[3 * vs + frow + fi];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int r = ty + 8 * q, i = i0 + r, j = j0 + tx;
    if (i < Hs && j < Ws) {
#pragma unroll
      for (int m = 0; m < 4; ++m) u[q][4 + m] = tile[m][tx * PITCH + r];
      const float* w = u[q];
      const float mu = (((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]))) * 0.125f;
      const long long o = pl * hw + (long long)i * Ws + j;
      mean[o] = mu;
      if constexpr (SPREAD) {
        float d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float t = w[k] - mu;
          d[k] = t * t;
        }
        const float var = (((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]))) * 0.125f;
        spread[o] = __fsqrt_rn(var);
      }
    }
  }
}

// min(max(v * s + 0.5f, 0.f), 255.f) truncated; the comparisons send a NaN to 0
__device__ __forceinline__ uint32_t to_u8(float v, float s) {
  float t = v * s + 0.5f;
  t = t > 0.f ? t : 0.f;
  t = t < 255.f ? t : 255.f;
  return (uint32_t)(int)t;
}

// planar float32 [C][n] -> interleaved uint8 [n][C], n = H * W: a thread owns four consecutive pixels = 4 C bytes = C aligned dwords of
// the destination; it reads four consecutive floats of each plane (one 16-byte load where the planes are 16-byte aligned).
// flags: 1 = 16-byte loads allowed, 2 = dword stores allowed (dst 4-byte aligned); the last, partial group goes byte by byte.
template <int C>
__global__ __launch_bounds__(256) void tensor_to_image_u8_kernel(const float* __restrict__ src, long long n, float s,
                                                                 uint8_t* __restrict__ dst, int flags) {
  const long long p0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
  if (p0 >= n) return;
  if (p0 + 4 <= n && (flags & 2)) {
    uint32_t bytes[4 * C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float* p = src + c * n + p0;
      float v[4];
      if (flags & 1) {
        load4(p, v);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) bytes[e * C + c] = to_u8(v[e], s);
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(dst + p0 * C);
#pragma unroll
    for (int w = 0; w < C; ++w)
      out[w] = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) | (bytes[4 * w + 3] << 24);
  } else {
    const long long p1 = p0 + 4 < n ? p0 + 4 : n;
    for (long long p = p0; p < p1; ++p)
#pragma unroll
      for (int c = 0; c < C; ++c) dst[p * C + c] = (uint8_t)to_u8(src[c * n + p], s);
  }
}

const char* plane_args(const void* p0, const void* p1, const void* p2, int planes, int H, int W) {
  if (!p0 || !p1 || !p2) return "null pointer";
  if (planes < 1 || planes > MAX_PLANES) return "planes must be 1 .. 65535";
  if (H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return "sides must be 1 .. 16384";
  return nullptr;
}

}  // namespace

extern "C" int m2t_dihedral_pack(const float* src, int planes, int H, int W, float* dst_a, float* dst_b, void* stream) {
  if (const char* bad = plane_args(src, dst_a, dst_b, planes, H, W)) return m2t_set_error_at(M2T_ERR_ARG, "m2t_dihedral_pack", bad);
  const dim3 grid(ceil_div(W, TILE), ceil_div(H, TILE), planes);
  dihedral_pack_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(src, planes, H, W, dst_a, dst_b);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" int m2t_dihedral_merge(const float* sr_a, const float* sr_b, int planes, int Hs, int Ws, float* mean, float* spread,
                                  void* stream) {
  if (const char* bad = plane_args(sr_a, sr_b, mean, planes, Hs, Ws)) return m2t_set_error_at(M2T_ERR_ARG, "m2t_dihedral_merge", bad);
  const dim3 grid(ceil_div(Ws, TILE), ceil_div(Hs, TILE), planes);
  if (spread) dihedral_merge_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(sr_a, sr_b, planes, Hs, Ws, mean, spread);
  else dihedral_merge_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(sr_a, sr_b, planes, Hs, Ws, mean, nullptr);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" int m2t_tensor_to_image_u8(const float* src, int channels, int H, int W, float rgb_range, unsigned char* dst, void* stream) {
  const char* bad = nullptr;
  if (!src || !dst) bad = "null pointer";
  else if (channels != 1 && channels != 3) bad = "channels must be 1 or 3";
  else if (H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) bad = "sides must be 1 .. 16384";
  else if (!isfinite(rgb_range) || !(rgb_range > 0.f)) bad = "rgb_range must be a finite number > 0";
  if (bad) return m2t_set_error_at(M2T_ERR_ARG, "m2t_tensor_to_image_u8", bad);
  const long long n = (long long)H * W;
  const float s = 255.0f / rgb_range;
  const int flags = ((((uintptr_t)src & 15) == 0 && (n & 3) == 0) ? 1 : 0) | ((((uintptr_t)dst & 3) == 0) ? 2 : 0);
  const int grid = (int)ceil_divll(ceil_divll(n, 4), 256);
  if (channels == 3) tensor_to_image_u8_kernel<3><<<grid, 256, 0, (hipStream_t)stream>>>(src, n, s, dst, flags);
  else tensor_to_image_u8_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(src, n, s, dst, flags);
  M2T_LAUNCH_CHECK();
  return 0;
}
