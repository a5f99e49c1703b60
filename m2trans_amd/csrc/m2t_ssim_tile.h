// m2t_ssim_tile.h -- the structural loss terms on the moment tile (m2t_moment_tile.h), shared by k_ssim_loss.hip (1 - SSIM) and
// k_msssim_loss.hip (MS-SSIM: the same map on five pooled levels, the contrast-structure variant on the first four).
//
// One workgroup owns a TS x TS tile of the image plane under the 11-tap window (TM = TS + 10, TI = TS + 20).  maps() leaves the three
// coefficient maps dM | dE | dF in LDS and returns the workgroup's sum over the map entries the tile owns.  grad() filters them back
// and hands d sum(map) / dx_normalised(q) of each of the tile's pixels to the caller's epilogue: one call per pixel, by one thread.
// What this header adds to the tile: the clamp where a value is used and its mask, the point-wise map, the last line of the gradient.
//
//   MAP_SSIM_LOSS, MAP_SSIM:  S = A1 A2 / (B1 B2);  dE = -S / B2, dF = 2 A1 / (B1 B2), dM = 2 m2 (A2 - A1) / (B1 B2) - 2 m1 S / B1 + 2 m1 S / B2
//   MAP_CS:                   cs = A2 / B2;         dE = -cs / B2, dF = 2 / B2,        dM = (-2 m2 + 2 m1 cs) / B2
//   (the summed quantity is 1 - S for MAP_SSIM_LOSS, the map itself for the other two)
//
// Everything between the inputs (fp32 widened, or fp64) and the epilogue is fp64 (k_ssim_loss.hip says why).  Inputs are
// UN-normalised: the 1 / R factors are applied to the moments.  TIn = float with TS = 32 and 512 threads is the tile of the SSIM
// term (151 392 B of LDS, one workgroup per CU); TIn = double needs a smaller tile (TS = 16, 256 threads: 74 464 B, two per CU).
#ifndef M2T_SSIM_TILE_H
#define M2T_SSIM_TILE_H
#include <hip/hip_runtime.h>
#include "m2t_moment_tile.h"

namespace ssim_tile {

using moment_tile::block_sum;

constexpr int WIN = 11;
struct Taps { double g[WIN]; };
enum MapKind { MAP_SSIM_LOSS = 0, MAP_SSIM = 1, MAP_CS = 2 };

__device__ __forceinline__ float clamp_to(float v, float R) { return fminf(fmaxf(v, 0.f), R); }
__device__ __forceinline__ double clamp_to(double v, double R) { return fmin(fmax(v, 0.0), R); }

template <typename TIn, int TS_, int NT_>
struct Tile : moment_tile::Tile<WIN, TS_, NT_, TIn> {
  using Base = moment_tile::Tile<WIN, TS_, NT_, TIn>;
  using In = TIn;

  // xp / yp: the [H][W] planes with row strides xs_row / ys_row; (y0, x0): the tile's first pixel.  SUM = false skips the
  // reduction (the return value is then meaningless); either way D is complete and V free for every thread on return.
  template <int KIND, bool SUM>
  static __device__ __forceinline__ double maps(unsigned char* smem, const TIn* __restrict__ xp, int xs_row, const TIn* __restrict__ yp,
                                                int ys_row, int H, int W, int y0, int x0, TIn R, int clamp, const Taps& win) {
    const double iR = 1.0 / (double)R, iR2 = iR * iR;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double sum[1] = {0.0};
    Base::template maps<SUM>(
        smem, H, W, y0, x0, win,
        [=](int gy, int gxx, TIn& a, TIn& b) {
          a = xp[(long long)gy * xs_row + gxx];
          b = yp[(long long)gy * ys_row + gxx];
        },
        // u = clamp(x), applied where a value is used: the mask of the gradient needs the raw one
        [=](TIn a) { return (double)(clamp ? clamp_to(a, R) : a); },
        [=](const double(&m)[5], bool valid, bool owned, double(&d)[3], double(&acc)[1]) {
          const double m1 = m[0] * iR, m2 = m[1] * iR;
          const double s1 = m[2] * iR2 - m1 * m1, s2 = m[3] * iR2 - m2 * m2, s12 = m[4] * iR2 - m1 * m2;
          const double A2 = 2.0 * s12 + C2, B2 = s1 + s2 + C2;
          double S, dM, dE, dF;
          if (KIND == MAP_CS) {
            S = A2 / B2;
            dM = (-2.0 * m2 + 2.0 * m1 * S) / B2;
            dE = -S / B2;
            dF = 2.0 / B2;
          } else {
            const double A1 = 2.0 * m1 * m2 + C1, B1 = m1 * m1 + m2 * m2 + C1;
            const double iB = 1.0 / (B1 * B2);
            S = A1 * A2 * iB;
            dM = 2.0 * m2 * (A2 - A1) * iB - 2.0 * m1 * S / B1 + 2.0 * m1 * S / B2;
            dE = -S / B2;
            dF = 2.0 * A1 * iB;
          }
          d[0] = valid ? dM : 0.0;
          d[1] = valid ? dE : 0.0;
          d[2] = valid ? dF : 0.0;
          if (owned) acc[0] += KIND == MAP_SSIM_LOSS ? 1.0 - S : S;
        },
        sum);
    return sum[0];
  }

  // After maps(): epi(gy, gxx, d, u_raw) for every pixel of the tile inside the image that the clamp passes (inclusive ends, as
  // the pixel losses; every pixel with clamp = 0), d = d sum(map) / dx_normalised(gy, gxx), u_raw the raw input there.
  template <typename Epi>
  static __device__ __forceinline__ void grad(unsigned char* smem, int H, int W, int y0, int x0, TIn R, int clamp, const Taps& win,
                                              Epi epi) {
    const double iR = 1.0 / (double)R;
    Base::grad(
        smem, H, W, y0, x0, win, [=](TIn uf) { return !clamp || (uf >= (TIn)0 && uf <= R); },      // the clamp passes no gradient
        [=](int gy, int gxx, double a0, double a1, double a2, TIn uf, TIn vf) {
          const double xn = (double)uf * iR, yn = (double)vf * iR;
          epi(gy, gxx, a0 + 2.0 * xn * a1 + yn * a2, uf);
        });
  }
};

}  // namespace ssim_tile
#endif
