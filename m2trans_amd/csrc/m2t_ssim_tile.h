// m2t_ssim_tile.h -- the tile machinery of the structural loss terms, shared by k_ssim_loss.hip (1 - SSIM) and k_msssim_loss.hip
// (MS-SSIM: the same map on five pooled levels, the contrast-structure variant on the first four).
//
// One workgroup owns a TS x TS tile of the image plane.  maps() loads the TI x TI input tile of both images (TI = TS + 20) into
// LDS, filters u, v, uu, vv, uv vertically then horizontally on the TM x TM map entries whose windows touch the tile (TM = TS + 10),
// leaves the three coefficient maps dM | dE | dF in LDS (0 outside the map: the zero extension of the transposed filter) and
// returns the workgroup's sum over the map entries whose top-left pixel the tile owns.  grad() filters the coefficient maps back
// and hands d sum(map) / dx_normalised(q) of each of the tile's pixels to the caller's epilogue: one call per pixel, by one thread.
//
//   MAP_SSIM_LOSS, MAP_SSIM:  S = A1 A2 / (B1 B2);  dE = -S / B2, dF = 2 A1 / (B1 B2), dM = 2 m2 (A2 - A1) / (B1 B2) - 2 m1 S / B1 + 2 m1 S / B2
//   MAP_CS:                   cs = A2 / B2;         dE = -cs / B2, dF = 2 / B2,        dM = (-2 m2 + 2 m1 cs) / B2
//   (the summed quantity is 1 - S for MAP_SSIM_LOSS, the map itself for the other two)
//
// Everything between the inputs (fp32 widened, or fp64) and the epilogue is fp64 (k_ssim_loss.hip says why).  Inputs are
// UN-normalised: the 1 / R factors are applied to the moments.  TIn = float with TS = 32 and 512 threads is the tile of the SSIM
// term (151 392 B of LDS, one workgroup per CU); TIn = double needs a smaller tile (TS = 16, 256 threads: 74 432 B, two per CU).
#ifndef M2T_SSIM_TILE_H
#define M2T_SSIM_TILE_H
#include <hip/hip_runtime.h>

namespace ssim_tile {

constexpr int WIN = 11;
struct Taps { double g[WIN]; };
enum MapKind { MAP_SSIM_LOSS = 0, MAP_SSIM = 1, MAP_CS = 2 };

template <int N>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < N / 64; ++w) t += red[w];
  return t;
}

__device__ __forceinline__ float clamp_to(float v, float R) { return fminf(fmaxf(v, 0.f), R); }
__device__ __forceinline__ double clamp_to(double v, double R) { return fmin(fmax(v, 0.0), R); }

template <typename TIn, int TS_, int NT_>
struct Tile {
  using In = TIn;
  static constexpr int TS = TS_;                // output tile edge (pixels)
  static constexpr int NT = NT_;                // threads per workgroup
  static constexpr int TM = TS + WIN - 1;       // map entries per tile edge whose windows touch the tile
  static constexpr int TI = TM + WIN - 1;       // input samples per tile edge
  // LDS (bytes): V = vertical pass of x, y, xx, yy, xy, later (aliased) the vertical pass of the transposed filter;
  // D = dM | dE | dF; the raw x | y tiles.
  static constexpr size_t OFF_V = 0;
  static constexpr size_t OFF_D = OFF_V + sizeof(double) * 5 * TM * TI;
  static constexpr size_t OFF_RED = OFF_D + sizeof(double) * 3 * TM * TM;
  static constexpr size_t OFF_X = OFF_RED + sizeof(double) * (NT / 64);
  static constexpr size_t OFF_Y = OFF_X + sizeof(TIn) * TI * TI;
  static constexpr size_t SMEM = OFF_Y + sizeof(TIn) * TI * TI;
  static_assert(SMEM <= 160 * 1024, "the tile does not fit the LDS of a CU");
  static_assert(3 * TS * TM <= 5 * TM * TI, "the transposed vertical pass is aliased on V");

  // xp / yp: the [H][W] planes with row strides xs_row / ys_row; (y0, x0): the tile's first pixel.  SUM = false skips the
  // reduction (the return value is then meaningless); either way D is complete and V free for every thread on return.
  template <int KIND, bool SUM>
  static __device__ __forceinline__ double maps(unsigned char* smem, const TIn* __restrict__ xp, int xs_row, const TIn* __restrict__ yp,
                                                int ys_row, int H, int W, int y0, int x0, TIn R, int clamp, const Taps& win) {
    double* const V = (double*)(smem + OFF_V);
    double* const D = (double*)(smem + OFF_D);
    double* const red = (double*)(smem + OFF_RED);
    TIn* const XR = (TIn*)(smem + OFF_X);
    TIn* const YR = (TIn*)(smem + OFF_Y);
    const int tid = threadIdx.x;
    const int Hm = H - WIN + 1, Wm = W - WIN + 1;
    const int my0 = y0 - (WIN - 1), mx0 = x0 - (WIN - 1);      // image / map coordinates of local index 0 (may be negative)

    // 1. the input tiles, raw (the clamp is applied where a value is used: the mask of the gradient needs the raw one); 0 outside the image
    for (int i = tid; i < TI * TI; i += NT) {
      const int r = i / TI, cc = i - r * TI;
      const int gy = my0 + r, gxx = mx0 + cc;
      const bool in = gy >= 0 && gy < H && gxx >= 0 && gxx < W;
      XR[i] = in ? xp[(long long)gy * xs_row + gxx] : (TIn)0;
      YR[i] = in ? yp[(long long)gy * ys_row + gxx] : (TIn)0;
    }
    __syncthreads();

    // 2. vertical pass of u, v, uu, vv, uv (u = clamp(x), v = y: unnormalised, the 1 / R factors are applied to the moments)
    for (int i = tid; i < TM * TI; i += NT) {
      const int r = i / TI, cc = i - r * TI;
      double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
#pragma unroll
      for (int t = 0; t < WIN; ++t) {
        TIn uf = XR[(r + t) * TI + cc];
        if (clamp) uf = clamp_to(uf, R);
        const double g = win.g[t], u = (double)uf, v = (double)YR[(r + t) * TI + cc];
        a0 = fma(g, u, a0); a1 = fma(g, v, a1); a2 = fma(g, u * u, a2); a3 = fma(g, v * v, a3); a4 = fma(g, u * v, a4);
      }
      V[0 * TM * TI + i] = a0; V[1 * TM * TI + i] = a1; V[2 * TM * TI + i] = a2; V[3 * TM * TI + i] = a3; V[4 * TM * TI + i] = a4;
    }
    __syncthreads();

    // 3. horizontal pass, the map and its three coefficient maps (0 outside the map: the zero extension of the transposed filter)
    const double iR = 1.0 / (double)R, iR2 = iR * iR;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double acc = 0.0;
    for (int i = tid; i < TM * TM; i += NT) {
      const int r = i / TM, cc = i - r * TM;
      double m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double a = 0;
#pragma unroll
        for (int t = 0; t < WIN; ++t) a = fma(win.g[t], V[q * TM * TI + r * TI + cc + t], a);
        m[q] = a;
      }
      const int py = my0 + r, px = mx0 + cc;
      const bool valid = py >= 0 && py < Hm && px >= 0 && px < Wm;
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
      D[0 * TM * TM + i] = valid ? dM : 0.0;
      D[1 * TM * TM + i] = valid ? dE : 0.0;
      D[2 * TM * TM + i] = valid ? dF : 0.0;
      if (valid && r >= WIN - 1 && cc >= WIN - 1) acc += KIND == MAP_SSIM_LOSS ? 1.0 - S : S;      // the map entries this tile owns
    }
    if (SUM) return block_sum<NT>(acc, red);                           // (its barriers also close D and free V)
    __syncthreads();
    return 0.0;
  }

  // After maps(): epi(gy, gxx, d, u_raw) for every pixel of the tile inside the image that the clamp passes (inclusive ends, as
  // the pixel losses; every pixel with clamp = 0), d = d sum(map) / dx_normalised(gy, gxx), u_raw the raw input there.
  template <typename Epi>
  static __device__ __forceinline__ void grad(unsigned char* smem, int H, int W, int y0, int x0, TIn R, int clamp, const Taps& win,
                                              Epi epi) {
    double* const T = (double*)(smem + OFF_V);
    const double* const D = (const double*)(smem + OFF_D);
    const TIn* const XR = (const TIn*)(smem + OFF_X);
    const TIn* const YR = (const TIn*)(smem + OFF_Y);
    const int tid = threadIdx.x;
    const double iR = 1.0 / (double)R;

    // 4. transposed filter, vertical: pixel row y0 + r collects the map rows y0 + r - t (local r + 10 - t)
    for (int i = tid; i < TS * TM; i += NT) {
      const int r = i / TM, cc = i - r * TM;
      double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
      for (int t = 0; t < WIN; ++t) {
        const double g = win.g[t];
        const int j = (r + WIN - 1 - t) * TM + cc;
        a0 = fma(g, D[j], a0); a1 = fma(g, D[TM * TM + j], a1); a2 = fma(g, D[2 * TM * TM + j], a2);
      }
      T[i] = a0; T[TS * TM + i] = a1; T[2 * TS * TM + i] = a2;
    }
    __syncthreads();

    // 5. transposed filter, horizontal; the gradient of this tile's pixels
    for (int i = tid; i < TS * TS; i += NT) {
      const int r = i / TS, cc = i - r * TS;
      const int gy = y0 + r, gxx = x0 + cc;
      if (gy >= H || gxx >= W) continue;
      const TIn uf = XR[(r + WIN - 1) * TI + cc + WIN - 1];
      if (clamp && !(uf >= (TIn)0 && uf <= R)) continue;               // the clamp passes no gradient
      double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
      for (int t = 0; t < WIN; ++t) {
        const double g = win.g[t];
        const int j = r * TM + cc + WIN - 1 - t;
        a0 = fma(g, T[j], a0); a1 = fma(g, T[TS * TM + j], a1); a2 = fma(g, T[2 * TS * TM + j], a2);
      }
      const double xn = (double)uf * iR, yn = (double)YR[(r + WIN - 1) * TI + cc + WIN - 1] * iR;
      epi(gy, gxx, a0 + 2.0 * xn * a1 + yn * a2, uf);
    }
  }
};

}  // namespace ssim_tile
#endif
