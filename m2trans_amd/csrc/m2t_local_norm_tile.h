// m2t_local_norm_tile.h -- the per-thread text of the local-window InstanceNorm statistics (option "local_norm" of include/m2t.h,
// which has the definition; k_local_norm.hip launches it).  It sits in a header, as plain host + device functions without LDS or
// barriers, so that tests/local_norm_emulate.cpp runs the same text on the host.
//
// X is a 64-channel map in the chunked layout (4 chunks of 16 channels, each [B * H * W][16]: p64 of m2t_common.h).  Two passes:
//   hsum_segment    one thread = 4 channels x SEGX output columns of one row: S1 = sum x, S2 = sum x^2 over the row window
//                   [j, j + k_w), j = win_start(x).  The first column sums its k_w values in ascending order; every later
//                   column slides, S <- (S + x[j' + k_w - 1]) - x[j' - 1], and only where the window moves.  fp64 pairs
//                   {S1, S2} go to hs [4][B * H * W][16][2].
//   vapply_segment  one thread = 4 channels x SEGY output rows of one column: the same walk down the rows of hs over [i, i + k_h),
//                   then per pixel m = S1 / n, v = max(S2 / n - m^2, 0), r = 1 / sqrt(v + 1e-5) in fp64 and
//                   xn = T((float(x) - float(m)) * float(r)): the per-pixel mean / rstd never go to memory.
// SEGX / SEGY are constants, not functions of the batch or of the device: the order of every sum depends on the pixel's position in
// its image alone, so the bits of an image do not depend on the batch it is in.  No atomics; every element of hs and of xn is
// written by exactly one thread; hs is fully written by pass 1 before pass 2 reads it.
//
// Cost of the segments: pass 1 reads (k_w + 2 SEGX) / SEGX x-values per output (neighbours, served by the caches) and writes 16 B;
// pass 2 reads (k_h + 2 SEGY) / SEGY pairs of 16 B per output, x once, and writes xn once (DESIGN.md has the byte count).
#ifndef M2T_LOCAL_NORM_TILE_H
#define M2T_LOCAL_NORM_TILE_H
#include <hip/hip_runtime.h>
#include <math.h>

namespace ln_tile {

constexpr int SEGX = 32;        // output columns per thread of pass 1
constexpr int SEGY = 64;        // output rows per thread of pass 2
constexpr int CPL = 4;          // channels per thread: 8-byte (bf16) / 16-byte (fp32) loads of x, 64-byte runs of hs
constexpr double EPS = 1e-5;    // InstanceNorm2d's

template <typename T> struct Vec4 { typedef T type __attribute__((ext_vector_type(4))); };
typedef double f64x2 __attribute__((ext_vector_type(2)));

// first row / column of the window of output position y on an axis of length n, k = min(T, n): a left pad of (k - 1) / 2, clamped
__host__ __device__ inline int win_start(int y, int k, int n) {
  const int i = y - (k - 1) / 2;
  return i < 0 ? 0 : (i > n - k ? n - k : i);
}

template <typename T> __host__ __device__ inline void load_x4(const T* p, double (&v)[CPL]) {
  const typename Vec4<T>::type a = *reinterpret_cast<const typename Vec4<T>::type*>(p);
#pragma unroll
  for (int c = 0; c < CPL; ++c) v[c] = (double)(float)a[c];
}

// xr: channel c0 of pixel (row, 0) of the thread's chunk; o: the same element of hs (pairs).  Columns [x0, x1) of a row of W.
template <typename T> __host__ __device__ inline void hsum_segment(const T* xr, double* o, int x0, int x1, int W, int kw) {
  double s1[CPL], s2[CPL], a[CPL], d[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) s1[c] = s2[c] = 0.0;
  int j = win_start(x0, kw, W);
#pragma unroll 4
  for (int t = 0; t < kw; ++t) {
    load_x4(xr + (size_t)(j + t) * 16, a);
#pragma unroll
    for (int c = 0; c < CPL; ++c) { s1[c] += a[c]; s2[c] += a[c] * a[c]; }
  }
  for (int x = x0; x < x1; ++x) {
    const int jn = win_start(x, kw, W);
    if (jn != j) {                      // the window moved by one column: jn = j + 1
      load_x4(xr + (size_t)(jn + kw - 1) * 16, a);
      load_x4(xr + (size_t)j * 16, d);
#pragma unroll
      for (int c = 0; c < CPL; ++c) { s1[c] = (s1[c] + a[c]) - d[c]; s2[c] = (s2[c] + a[c] * a[c]) - d[c] * d[c]; }
      j = jn;
    }
    f64x2* q = reinterpret_cast<f64x2*>(o + (size_t)x * 32);
#pragma unroll
    for (int c = 0; c < CPL; ++c) q[c] = (f64x2){s1[c], s2[c]};
  }
}

// hc / xc / yc: channel c0 of pixel (0, x) of the thread's image and chunk in hs (pairs) / X / Xn.  Rows [y0, y1) of a column of H.
template <typename T>
__host__ __device__ inline void vapply_segment(const double* hc, const T* xc, T* yc, int y0, int y1, int H, int W, int kh, double n) {
  double s1[CPL], s2[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) s1[c] = s2[c] = 0.0;
  int i = win_start(y0, kh, H);
#pragma unroll 4
  for (int t = 0; t < kh; ++t) {
    const f64x2* q = reinterpret_cast<const f64x2*>(hc + (size_t)(i + t) * W * 32);
#pragma unroll
    for (int c = 0; c < CPL; ++c) { const f64x2 a = q[c]; s1[c] += a[0]; s2[c] += a[1]; }
  }
  for (int y = y0; y < y1; ++y) {
    const int in = win_start(y, kh, H);
    if (in != i) {
      const f64x2* qa = reinterpret_cast<const f64x2*>(hc + (size_t)(in + kh - 1) * W * 32);
      const f64x2* qd = reinterpret_cast<const f64x2*>(hc + (size_t)i * W * 32);
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const f64x2 a = qa[c], d = qd[c];
        s1[c] = (s1[c] + a[0]) - d[0];
        s2[c] = (s2[c] + a[1]) - d[1];
      }
      i = in;
    }
    const typename Vec4<T>::type xv = *reinterpret_cast<const typename Vec4<T>::type*>(xc + (size_t)y * W * 16);
    typename Vec4<T>::type out;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const double m = s1[c] / n;
      double v = s2[c] / n - m * m;
      v = v > 0.0 ? v : 0.0;
      const double r = 1.0 / sqrt(v + EPS);
      const float mean32 = (float)m, rstd32 = (float)r;
      const float df = (float)xv[c] - mean32;
      out[c] = (T)(df * rstd32);
    }
    *reinterpret_cast<typename Vec4<T>::type*>(yc + (size_t)y * W * 16) = out;
  }
}

}  // namespace ln_tile
#endif
