// k_resize.hip -- MATLAB-style imresize(..., 'bicubic') by an integer factor 2, 3 or 4 (include/m2t_resize.h): the LR half of the
// datasets (the reference's offline `_LR_bicubic` folders, datas/us1k.py:84,176, datas/benchmark.py) and the Bicubic baseline row.
//
// One fused kernel family, templated on element type (uint8 HWC interleaved / fp32 planar), factor and direction.  Along one axis an
// output "cell" q reads the NT inputs q * SIN + M0 + t, t = 0 .. NT-1, and produces SOUT outputs q * SOUT + p:
//   down  SIN = s, SOUT = 1, one filter of NT = 8 / 11 / 16 taps from M0 = -3 / -4 / -6 (x3 holds two exact zeros: 9 non-zero);
//   up    SIN = 1, SOUT = s, s phases of NT = 5 taps from M0 = -2 (the four taps of a phase and one exact zero at either end).
// The normalised fp64 taps are computed on the host and travel in the kernel arguments: no table allocation, no upload.
//
// A workgroup (256 threads) owns one output tile of TQH x TQW cells.  It loads the input tile with its mirrored halo into LDS once
// (element type kept: bytes stay bytes), then runs, per strip of SRQ cell rows, the vertical pass into an fp64 LDS strip and the
// horizontal pass out of it, and stores the strip: no intermediate goes to HBM, nothing is rounded between the passes.  The strip
// is what makes x4 down fit: its byte tile is 76 x 140 x 3 = 31,920 B and the fp64 intermediate of all 16 rows would be 53,760 B;
// 8 rows are 26,880 B, 58,800 B in all (the phase table exists in the up kernels only): two workgroups per CU (LDS budget per
// instantiation: DESIGN.md).
// uint8: global bytes are fetched as aligned dwords over the in-image part of each tile row (the halo, a few pixels, byte-wise
// through the mirror), LDS is read a dword = 4 elements per lane in the vertical pass, and the result is written as aligned packed
// dwords (single bytes only at the ragged ends of a row).  fp64 accumulation, no atomics: two runs are bit-identical.
#include "m2t_common.h"
#include "../../include/m2t_resize.h"
#include <math.h>

namespace {

constexpr int MAX_TAPS = 20;                   // 16 (x4 down) / 4 phases x 5 (x4 up)
struct Taps { double w[MAX_TAPS]; };           // [phase][tap]

template <int S, bool UP> struct Geo {
  static constexpr int SIN = UP ? 1 : S, SOUT = UP ? S : 1;
  static constexpr int NT = UP ? 5 : (S == 2 ? 8 : S == 3 ? 11 : 16);
  static constexpr int M0 = UP ? -2 : (S == 2 ? -3 : S == 3 ? -4 : -6);
  static constexpr int TQH = 16, TQW = UP ? 16 : 32;      // cells per tile
  static constexpr int SRQ = UP ? 16 : 8;                 // cell rows per strip
  static constexpr int IH = (TQH - 1) * SIN + NT, IW = (TQW - 1) * SIN + NT;
};

// MATLAB's aux = [1:n, n:-1:1] on 0-based indices: period 2n, edge pixel repeated; any j (the halo may wrap a short axis often)
__device__ __forceinline__ int mirror_idx(int j, int n) {
  const int p = 2 * n;
  int m = j % p;
  m += (m >> 31) & p;
  return min(m, p - 1 - m);
}

template <typename T> __device__ __forceinline__ T finish(double v, float clamp_max);
template <> __device__ __forceinline__ uint8_t finish<uint8_t>(double v, float) {
  return (uint8_t)(int)fmin(fmax(round(v), 0.0), 255.0);            // half away from zero, then saturate
}
template <> __device__ __forceinline__ float finish<float>(double v, float clamp_max) {
  if (clamp_max > 0.f) v = fmin(fmax(v, 0.0), (double)clamp_max);
  return (float)v;
}

// grid (tiles along W, tiles along H, planes)
template <typename T, int CH, int S, bool UP>
__global__ __launch_bounds__(256) void imresize_kernel(const T* __restrict__ src, T* __restrict__ dst, int H, int W, int OH, int OW,
                                                       Taps taps, float clamp_max) {
  using G = Geo<S, UP>;
  constexpr int SIN = G::SIN, SOUT = G::SOUT, NT = G::NT;
  constexpr int EPT = sizeof(T) == 1 ? 4 : 1;               // elements per lane and LDS access: one dword
  constexpr int IWE = G::IW * CH;                           // elements of a tile row
  constexpr int PITCH = (IWE + EPT - 1) / EPT * EPT;
  constexpr int NG = PITCH / EPT;
  constexpr int MROWS = G::SRQ * SOUT;                      // output rows per strip
  __shared__ __attribute__((aligned(16))) T tile[G::IH * PITCH];
  __shared__ double mid[MROWS * PITCH];
  __shared__ double wl[MAX_TAPS];

  const int tid = threadIdx.x;
  const int qy0 = blockIdx.y * G::TQH, qx0 = blockIdx.x * G::TQW;
  const int ys = qy0 * SIN + G::M0, xs = qx0 * SIN + G::M0;
  const T* img = src + (long long)blockIdx.z * H * W * CH;
  T* out = dst + (long long)blockIdx.z * OH * OW * CH;
  if constexpr (UP) {
#pragma unroll
    for (int i = 0; i < SOUT * NT; ++i)
      if (tid == i) wl[i] = taps.w[i];
  }

  // ---- input tile with its mirrored halo
  if constexpr (sizeof(T) == 1) {
    const int cx0 = max(xs, 0), cx1 = min(xs + G::IW, W);   // the in-image pixel columns of the tile
    const int nb = (cx1 - cx0) * CH;                        // ... as bytes of a row
    constexpr int NDW = IWE / 4 + 2;
    for (int i = tid; i < G::IH * NDW; i += 256) {
      const int r = i / NDW, d = i - r * NDW;
      const int sy = mirror_idx(ys + r, H);
      const uint8_t* rowp = img + ((long long)sy * W + cx0) * CH;
      const int b = 4 * d - (int)((uintptr_t)rowp & 3);     // byte offset of the d-th ALIGNED dword that touches the row part
      if (b >= nb) continue;
      uint8_t* lp = tile + r * PITCH + (cx0 - xs) * CH + b;
      if (b >= 0 && b + 4 <= nb) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(rowp + b);
        lp[0] = (uint8_t)v; lp[1] = (uint8_t)(v >> 8); lp[2] = (uint8_t)(v >> 16); lp[3] = (uint8_t)(v >> 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (b + k >= 0 && b + k < nb) lp[k] = rowp[b + k];
      }
    }
    const int nl = cx0 - xs, nh = nl + (xs + G::IW - cx1);  // halo pixels left of / in all beside the in-image part
    for (int i = tid; i < G::IH * nh * CH; i += 256) {
      const int r = i / (nh * CH), j = i - r * (nh * CH);
      const int h = j / CH, c = j - h * CH;
      const int x = h < nl ? h : (cx1 - xs) + (h - nl);
      const int sy = mirror_idx(ys + r, H), sx = mirror_idx(xs + x, W);
      tile[r * PITCH + x * CH + c] = img[((long long)sy * W + sx) * CH + c];
    }
  } else {
    for (int i = tid; i < G::IH * IWE; i += 256) {
      const int r = i / IWE, x = i - r * IWE;
      const int sy = mirror_idx(ys + r, H), sx = mirror_idx(xs + x, W);
      tile[r * PITCH + x] = img[(long long)sy * W + sx];
    }
  }
  __syncthreads();

  const int olen = min(G::TQW * SOUT, OW - qx0 * SOUT) * CH;            // elements of this tile's output rows
  constexpr int NGO = (G::TQW * SOUT * CH + EPT - 1) / EPT + (EPT > 1 ? 1 : 0);
  for (int s0 = 0; s0 < G::TQH; s0 += G::SRQ) {
    // ---- vertical pass: tile rows -> fp64 strip, EPT neighbouring elements per lane
    for (int i = tid; i < G::SRQ * NG; i += 256) {
      const int qq = i / NG, g = i - qq * NG;
      const T* col = tile + (s0 + qq) * SIN * PITCH + g * EPT;
      double acc[SOUT][EPT];
#pragma unroll
      for (int p = 0; p < SOUT; ++p)
#pragma unroll
        for (int e = 0; e < EPT; ++e) acc[p][e] = 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        double v[EPT];
        if constexpr (sizeof(T) == 1) {
          const uint32_t u = *reinterpret_cast<const uint32_t*>(col + t * PITCH);
#pragma unroll
          for (int e = 0; e < EPT; ++e) v[e] = (double)((u >> (8 * e)) & 255u);
        } else {
          v[0] = (double)col[t * PITCH];
        }
#pragma unroll
        for (int p = 0; p < SOUT; ++p)
#pragma unroll
          for (int e = 0; e < EPT; ++e) acc[p][e] += taps.w[p * NT + t] * v[e];
      }
#pragma unroll
      for (int p = 0; p < SOUT; ++p)
#pragma unroll
        for (int e = 0; e < EPT; ++e) mid[(qq * SOUT + p) * PITCH + g * EPT + e] = acc[p][e];
    }
    __syncthreads();
    // ---- horizontal pass: fp64 strip -> output rows, EPT neighbouring output elements per lane, dword-aligned in HBM for uint8
    for (int i = tid; i < MROWS * NGO; i += 256) {
      const int mr = i / NGO, k = i - mr * NGO;
      const int oy = (qy0 + s0) * SOUT + mr;
      if (oy >= OH) continue;
      T* orow = out + ((long long)oy * OW + (long long)qx0 * SOUT) * CH;
      const int e0 = k * EPT - (EPT > 1 ? (int)((uintptr_t)orow & 3) : 0);
      if (e0 >= olen) continue;
      T res[EPT];
#pragma unroll
      for (int j = 0; j < EPT; ++j) {
        const int e = e0 + j;
        res[j] = T(0);
        if (e < 0 || e >= olen) continue;
        const int px = e / CH, c = e - px * CH;
        const int q = px / SOUT, p = px - q * SOUT;
        const double* m = mid + mr * PITCH + q * SIN * CH + c;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          double w;
          if constexpr (UP) w = wl[p * NT + t]; else w = taps.w[t];
          acc += w * m[t * CH];
        }
        res[j] = finish<T>(acc, clamp_max);
      }
      if constexpr (EPT == 4) {
        if (e0 >= 0 && e0 + 4 <= olen) {
          *reinterpret_cast<uint32_t*>(orow + e0) = (uint32_t)res[0] | ((uint32_t)res[1] << 8) | ((uint32_t)res[2] << 16) | ((uint32_t)res[3] << 24);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (e0 + j >= 0 && e0 + j < olen) orow[e0 + j] = res[j];
        }
      } else {
        orow[e0] = res[0];
      }
    }
    __syncthreads();
  }
}

// cubic convolution kernel, a = -0.5 (the expression order is the one of resize.filter_taps)
double cubic(double x) {
  x = fabs(x);
  if (x <= 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
  if (x <= 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
  return 0.0;
}

template <int S, bool UP> Taps make_taps() {
  using G = Geo<S, UP>;
  Taps tp;
  for (int i = 0; i < MAX_TAPS; ++i) tp.w[i] = 0.0;
  for (int p = 0; p < G::SOUT; ++p) {
    double* w = tp.w + p * G::NT;
    double sum = 0.0;
    for (int t = 0; t < G::NT; ++t) {
      const int m = G::M0 + t;
      // u - j from its exact integer numerator over 2 s (one rounding): up u = q + (p + 1/2) / s - 1/2, j = q + m; down d / s with
      // d = (s - 1) / 2 - m
      if (UP) w[t] = cubic((2 * p + 1 - S - 2 * S * m) / (2.0 * S));
      else w[t] = cubic((S - 1 - 2 * m) / (2.0 * S)) / S;
      sum += w[t];
    }
    for (int t = 0; t < G::NT; ++t) w[t] /= sum;
  }
  return tp;
}

template <typename T, int CH, int S, bool UP>
int launch(const T* src, int planes, int H, int W, T* dst, int OH, int OW, float clamp_max, hipStream_t stream) {
  using G = Geo<S, UP>;
  const int qh = UP ? H : OH, qw = UP ? W : OW;
  const dim3 grid(ceil_div(qw, G::TQW), ceil_div(qh, G::TQH), planes);
  imresize_kernel<T, CH, S, UP><<<grid, 256, 0, stream>>>(src, dst, H, W, OH, OW, make_taps<S, UP>(), clamp_max);
  M2T_LAUNCH_CHECK();
  return 0;
}

template <typename T, int CH>
int dispatch(const char* who, const T* src, int planes, int H, int W, T* dst, int scale, int up, float clamp_max, void* stream) {
  char msg[160];
  const char* bad = nullptr;
  if (!src || !dst) bad = "null pointer";
  else if (scale < 2 || scale > 4) bad = "scale must be 2, 3 or 4";
  else if (H < 1 || W < 1) bad = "H and W must be at least 1";
  else if (!up && (H % scale || W % scale)) bad = "down: H and W must be multiples of scale";
  else if ((up ? (long long)H * scale : H / scale) > 16384 || (up ? (long long)W * scale : W / scale) > 16384) bad = "output side above 16384";
  if (bad) {
    snprintf(msg, sizeof msg, "%s: %s", who, bad);
    return m2t_set_error(M2T_ERR_ARG, msg);
  }
  const int OH = up ? H * scale : H / scale, OW = up ? W * scale : W / scale;
  hipStream_t st = (hipStream_t)stream;
  switch (scale * 2 + (up ? 1 : 0)) {
    case 4: return launch<T, CH, 2, false>(src, planes, H, W, dst, OH, OW, clamp_max, st);
    case 5: return launch<T, CH, 2, true>(src, planes, H, W, dst, OH, OW, clamp_max, st);
    case 6: return launch<T, CH, 3, false>(src, planes, H, W, dst, OH, OW, clamp_max, st);
    case 7: return launch<T, CH, 3, true>(src, planes, H, W, dst, OH, OW, clamp_max, st);
    case 8: return launch<T, CH, 4, false>(src, planes, H, W, dst, OH, OW, clamp_max, st);
    default: return launch<T, CH, 4, true>(src, planes, H, W, dst, OH, OW, clamp_max, st);
  }
}

}  // namespace

extern "C" int m2t_imresize_u8(const unsigned char* src, int H, int W, int channels, unsigned char* dst, int scale, int up, void* stream) {
  if (channels != 3) return m2t_set_error(M2T_ERR_ARG, "m2t_imresize_u8: channels must be 3");
  return dispatch<uint8_t, 3>("m2t_imresize_u8", src, 1, H, W, dst, scale, up, 0.f, stream);
}

extern "C" int m2t_imresize_f32(const float* src, int planes, int H, int W, float* dst, int scale, int up, float clamp_max, void* stream) {
  if (planes < 1 || planes > 65535) return m2t_set_error(M2T_ERR_ARG, "m2t_imresize_f32: planes must be 1 .. 65535");
  if (!isfinite(clamp_max)) return m2t_set_error(M2T_ERR_ARG, "m2t_imresize_f32: clamp_max must be finite");
  return dispatch<float, 1>("m2t_imresize_f32", src, planes, H, W, dst, scale, up, clamp_max, stream);
}
