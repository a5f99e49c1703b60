// m2t_vif_tile.h -- the tile machinery of the pixel-domain VIF loss term (k_vif_loss.hip; include/m2t_vif.h has the definition).
//
// VIF works on ONE luminance plane per image, on four scales s = 0 .. 3 with window lengths N_s = 17, 9, 5, 3; level s > 0 is the
// level above filtered with G_s (VALID) and decimated by 2.  Everything here is fp64; level 0 is formed from the fp32 images in the
// load (clamp, luminance weights, 255 / R), levels 1 .. 3 are fp64 planes.
//
//   pyr_tile<N, L0>   one 16 x 16 tile of level s from level s - 1: the raw (2 * 15 + N)^2 input tile in LDS, the vertical pass on the
//                     16 rows that survive the decimation only, the horizontal pass on the 16 surviving columns only.
//   Tile<N, TS, NT>   the moment tile (m2t_moment_tile.h) of a level under its N-tap window: TI = TS + 2 (N - 1) input samples and
//                     TM = TS + N - 1 map entries per edge.  maps() forms u and v in the load (level 0: clamp, luminance, 255 / R)
//                     and leaves the three coefficient maps in LDS -- dA = dt/da (on u^2), dC = dt/dc (on u v),
//                     dU = -2 mx dt/da - my dt/dc (on u); 0 outside the map and where the entry is not live -- and returns the tile's
//                     sums of t and d over the map entries it owns.  grad() filters the three maps back and hands
//                     d sum(t) / du_s(p) = 2 u(p) G^T[dA] + v(p) G^T[dC] + G^T[dU] of each of the tile's pixels to the epilogue.
//   parent_gather     the adjoint of (filter G_{s+1}, decimate) applied to the gradient of level s + 1, GATHERED for one pixel of
//                     level s: sum over the parents (i, j) with 0 <= p - 2 (i, j) < N_{s+1} of g[py - 2 i] g[px - 2 j] G_{s+1}(i, j).
//
// LDS per workgroup, TS = 16, 256 threads (V = 5 TM TI, D = 3 TM TM, raw u | v = 2 TI TI doubles, + 64 B):
//   N = 17: TM 32, TI 48: 122 944 B, one workgroup per CU      N = 9: TM 24, TI 32: 60 992 B, two per CU
//   N =  5: TM 20, TI 24:  38 080 B, four per CU               N = 3: TM 18, TI 20: 28 640 B, five per CU
// (a 32 x 32 tile under the 17-tap window would need 5 * 48 * 64 + 3 * 48 * 48 + 2 * 64 * 64 doubles = 243 712 B: it does not fit.)
#ifndef M2T_VIF_TILE_H
#define M2T_VIF_TILE_H
#include <hip/hip_runtime.h>
#include <math.h>
#include "m2t_ssim_tile.h"      // clamp_to; the moment tile comes with it

namespace vif_tile {

using moment_tile::block_sum;

constexpr int SCALES = 4;
constexpr int MAXWIN = 17;
constexpr int MIN_SIDE = 41;                   // the scale-3 map of a 41-pixel side is one entry
constexpr double EPS = 1e-8;
constexpr int win_len(int s) { return (1 << (4 - s)) + 1; }
constexpr int PT = 16;                         // output tile edge of the pyramid kernel

struct Taps { double g[MAXWIN]; };             // the first N are used

// g[k] = exp(-(k - (N - 1) / 2)^2 / (2 (N / 5)^2)) / sum, in fp64, summed in index order
inline void make_taps(int N, double* g) {
  const double sd = (double)N / 5.0, mid = (double)(N - 1) / 2.0;
  double sum = 0.0;
  for (int k = 0; k < N; ++k) {
    const double d = (double)k - mid;
    g[k] = exp(-(d * d) / (2.0 * sd * sd));
    sum += g[k];
  }
  for (int k = 0; k < N; ++k) g[k] = g[k] / sum;
}

// the level above / below: filtered VALID with N taps, every second sample from 0
inline int decimated_side(int n, int N) { return (n - N + 2) / 2; }

// Where a level of ONE image comes from.  Level 0: the fp32 images (x with channel / row strides, optionally clamped to [0, R]; y
// contiguous, never clamped) through u = k255 * ((0.299 r + 0.587 g) + 0.114 b), or k255 * the one channel.  Levels 1 .. 3: fp64 planes.
struct Src {
  const float* x; const float* y;
  long long xs_ch; int xs_row; long long ys_ch; int ys_row; int C; float R; int clamp; double k255;
  const double* u; const double* v; int row;
};

template <bool L0>
__device__ __forceinline__ void load_uv(const Src& s, int gy, int gxx, double& u, double& v) {
  if (L0) {
    const float* const xp = s.x + (long long)gy * s.xs_row + gxx;
    const float* const yp = s.y + (long long)gy * s.ys_row + gxx;
    float a0 = xp[0];
    if (s.clamp) a0 = ssim_tile::clamp_to(a0, s.R);
    if (s.C == 3) {
      float a1 = xp[s.xs_ch], a2 = xp[2 * s.xs_ch];
      if (s.clamp) { a1 = ssim_tile::clamp_to(a1, s.R); a2 = ssim_tile::clamp_to(a2, s.R); }
      u = s.k255 * ((0.299 * (double)a0 + 0.587 * (double)a1) + 0.114 * (double)a2);
      v = s.k255 * ((0.299 * (double)yp[0] + 0.587 * (double)yp[s.ys_ch]) + 0.114 * (double)yp[2 * s.ys_ch]);
    } else {
      u = s.k255 * (double)a0;
      v = s.k255 * (double)yp[0];
    }
  } else {
    u = s.u[(long long)gy * s.row + gxx];
    v = s.v[(long long)gy * s.row + gxx];
  }
}

// ---- the pyramid: level s (Ho x Wo) from level s - 1 (Hi x Wi), window N = N_s; 256 threads, tile (blockIdx.y, blockIdx.x) -----------
template <int N>
struct Pyr {
  static constexpr int PI = 2 * (PT - 1) + N;                        // input samples per tile edge
  static constexpr size_t SMEM = sizeof(double) * (2 * PI * PI + 2 * PT * PI);
};

template <int N, bool L0>
__device__ __forceinline__ void pyr_tile(unsigned char* smem, const Src& src, int Hi, int Wi, int Ho, int Wo, const Taps& win,
                                         double* __restrict__ uo, double* __restrict__ vo) {
  constexpr int PI = Pyr<N>::PI, NT = 256;
  double* const RU = (double*)smem;
  double* const RV = RU + PI * PI;
  double* const TU = RV + PI * PI;
  double* const TV = TU + PT * PI;
  const int tid = threadIdx.x;
  const int oy0 = blockIdx.y * PT, ox0 = blockIdx.x * PT;
  for (int i = tid; i < PI * PI; i += NT) {
    const int r = i / PI, cc = i - r * PI;
    const int gy = 2 * oy0 + r, gxx = 2 * ox0 + cc;
    double u = 0.0, v = 0.0;
    if (gy < Hi && gxx < Wi) load_uv<L0>(src, gy, gxx, u, v);
    RU[i] = u; RV[i] = v;
  }
  __syncthreads();
  for (int i = tid; i < PT * PI; i += NT) {                          // vertical, the surviving rows only
    const int r = i / PI, cc = i - r * PI;
    double a = 0, b = 0;
#pragma unroll
    for (int t = 0; t < N; ++t) {
      a = fma(win.g[t], RU[(2 * r + t) * PI + cc], a);
      b = fma(win.g[t], RV[(2 * r + t) * PI + cc], b);
    }
    TU[i] = a; TV[i] = b;
  }
  __syncthreads();
  for (int i = tid; i < PT * PT; i += NT) {                          // horizontal, the surviving columns only
    const int r = i / PT, cc = i - r * PT;
    const int oy = oy0 + r, ox = ox0 + cc;
    if (oy >= Ho || ox >= Wo) continue;
    double a = 0, b = 0;
#pragma unroll
    for (int t = 0; t < N; ++t) {
      a = fma(win.g[t], TU[r * PI + 2 * cc + t], a);
      b = fma(win.g[t], TV[r * PI + 2 * cc + t], b);
    }
    uo[(long long)oy * Wo + ox] = a;
    vo[(long long)oy * Wo + ox] = b;
  }
}

// ---- the adjoint of (filter, decimate), gathered: gp [Hp][Wp] is the gradient of level s + 1, g[NP] its window -----------------------
// (g points into LDS: the index depends on the pixel's parity, a private or kernel-argument array would go to scratch)
template <int NP>
__device__ __forceinline__ double parent_gather(const double* __restrict__ gp, int Hp, int Wp, const double* g, int py, int px) {
  const int i0 = py - NP + 1 > 0 ? (py - NP + 2) >> 1 : 0, i1 = (py >> 1) < Hp - 1 ? (py >> 1) : Hp - 1;
  const int j0 = px - NP + 1 > 0 ? (px - NP + 2) >> 1 : 0, j1 = (px >> 1) < Wp - 1 ? (px >> 1) : Wp - 1;
  double acc = 0.0;
  for (int i = i0; i <= i1; ++i) {
    const double gi = g[py - 2 * i];
    double row = 0.0;
    for (int j = j0; j <= j1; ++j) row = fma(g[px - 2 * j], gp[(long long)i * Wp + j], row);
    acc = fma(gi, row, acc);
  }
  return acc;
}

// ---- the moments, the map and its coefficient maps on one tile of one level: the moment tile with the luminance load, the
// five-branch map (sums of t and d) and 2 u G^T[dA] + v G^T[dC] + G^T[dU] ----------------------------------------------------------
template <int N_, int TS_, int NT_>
struct Tile : moment_tile::Tile<N_, TS_, NT_, double> {
  using Base = moment_tile::Tile<N_, TS_, NT_, double>;
  static constexpr int N = N_;

  // (y0, x0): the tile's first pixel; nn = sigma_n_sq.  SUM: sum_t / sum_d of the owned map entries are returned to every thread.
  template <bool L0, bool SUM>
  static __device__ __forceinline__ void maps(unsigned char* smem, const Src& src, int H, int W, int y0, int x0, double nn,
                                              const Taps& win, double& sum_t, double& sum_d) {
    const double iln10 = 0.43429448190325182765;        // 1 / ln 10
    double sum[2];
    Base::template maps<SUM>(
        smem, H, W, y0, x0, win, [&](int gy, int gxx, double& u, double& v) { load_uv<L0>(src, gy, gxx, u, v); },
        [](double u) { return u; },
        [=](const double(&m)[5], bool valid, bool owned, double(&d)[3], double(&acc)[2]) {
          const double mx = m[0], my = m[1];
          const double a = fmax(m[2] - mx * mx, 0.0), b = fmax(m[3] - my * my, 0.0), c = m[4] - mx * my;
          const bool live = valid && b >= EPS && a >= EPS && c >= 0.0;
          double t = 0.0, dA = 0.0, dC = 0.0;
          if (live) {
            const double be = b + EPS;
            const double g = c / be;
            const double sv_raw = a - g * c;
            const bool open = sv_raw > EPS;
            const double z = (open ? sv_raw : EPS) + nn;
            const double q = g * g * b;
            t = log10(1.0 + q / z);
            const double k = iln10 / (1.0 + q / z);
            const double qz2 = q / (z * z);
            dA = open ? -k * qz2 : 0.0;
            dC = k * (2.0 * c * b / (be * be * z) + qz2 * (open ? 2.0 * c / be : 0.0));
          }
          d[0] = dA;
          d[1] = dC;
          d[2] = -2.0 * mx * dA - my * dC;
          if (owned) {
            acc[0] += t;
            if (b >= EPS) acc[1] += log10(1.0 + b / nn);
          }
        },
        sum);
    if (SUM) { sum_t = sum[0]; sum_d = sum[1]; }
  }

  // After maps(): epi(gy, gxx, d) for every pixel of the tile inside the level, d = d sum(t) / du_s(gy, gxx), this scale's own part.
  template <typename Epi>
  static __device__ __forceinline__ void grad(unsigned char* smem, int H, int W, int y0, int x0, const Taps& win, Epi epi) {
    Base::grad(smem, H, W, y0, x0, win, [](double) { return true; },
               [=](int gy, int gxx, double a0, double a1, double a2, double u, double v) { epi(gy, gxx, 2.0 * u * a0 + v * a1 + a2); });
  }
};

}  // namespace vif_tile
#endif
