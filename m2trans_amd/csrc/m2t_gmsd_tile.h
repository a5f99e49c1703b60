// m2t_gmsd_tile.h -- the tile text of the GMSD loss term (k_gmsd_loss.hip; include/m2t_gmsd.h has the definition).  It sits in a header
// so that tests/gmsd_emulate.cpp runs the same text on host threads.
//
// GMSD works on ONE pooled luminance plane per image: u (of x, through the optional clamp) and v (of y), hp x wp = ceil(H / 2) x
// ceil(W / 2) cells of 2 x 2 pixels.  A workgroup of 256 threads owns a tile of TP x TP = 32 x 32 cells.  Everything behind the fp32
// pixels is fp64.
//
//   stage<HY>    u and v of the tile plus a halo of HY cell rows and HX = 2 cell columns into LDS, 0 outside the map (the zero padding
//                of the Prewitt pair) and for pixels outside the image (the pad to an even size).  The work item is a PAIR of cells
//                (even cell column, so pixel column % 4 == 0): per image, row and channel one 16-byte load where the alignment and the
//                image edge allow it, four guarded scalar loads elsewhere.  The halo is 2 columns wide in both phases to keep that
//                alignment; phase 1 uses one of them.
//   value_tile   phase 1: stage<1>, then d = (m - m')^2 / D of every cell of the tile inside the map; returns the tile's sums of d, d^2.
//   grad_tile    phase 2: stage<2>, then (a_x, a_y) on the tile plus 1 into LDS (0 outside the map and where m = 0), then the
//                transposed Prewitt pair per cell of the tile and the scatter to the 2 x 2 pixels x C channels through the clamp mask:
//                again per pair of cells, 16-byte loads of x and of the destination and one 16-byte store where allowed (an element the
//                mask holds back is then stored back with the bits it had), scalar read-add-write elsewhere.  Elements outside [H, W]
//                are never read or written.
//
// LDS: 64 B of reduction space | U, V: (TP + 2 HY) x 36 doubles each | AX, AY: 34 x 34 doubles each (phase 2 only).
//   phase 1: 64 + 2 * 34 * 36 * 8 = 19 648 B        phase 2: 64 + 2 * 36 * 36 * 8 + 2 * 34 * 34 * 8 = 39 296 B (four workgroups per CU)
#ifndef M2T_GMSD_TILE_H
#define M2T_GMSD_TILE_H
#include <hip/hip_runtime.h>
#include <math.h>
#include "m2t_moment_tile.h"    // block_sum

namespace gmsd_tile {

using moment_tile::block_sum;

constexpr int TP = 32;                         // cells per tile edge
constexpr int NT = 256;                        // threads per workgroup
constexpr int HX = 2;                          // halo columns staged (phase 1 needs 1, phase 2 needs 2; 2 keeps pairs aligned)
constexpr int LW = TP + 2 * HX;                // LDS row length of U and V
constexpr int AW = TP + 2;                     // edge of the (a_x, a_y) region
constexpr double T = 170.0 / (255.0 * 255.0);
constexpr size_t RED_BYTES = 64;
constexpr size_t smem_bytes(int hy, bool grad) {
  return RED_BYTES + sizeof(double) * (2 * (size_t)(TP + 2 * hy) * LW + (grad ? 2 * (size_t)AW * AW : 0));
}
constexpr size_t SMEM_VALUE = smem_bytes(1, false), SMEM_GRAD = smem_bytes(2, true);

struct alignas(16) F4 { float f[4]; };

// ONE image: x with channel / row strides (optionally clamped to [0, R]), y contiguous (never clamped).  vec_x / vec_y: every row of
// every channel starts on a 16-byte boundary (decided on the host from the pointers and the strides); gx has x's strides and alignment.
struct Src {
  const float* x; const float* y;
  long long xs_ch; int xs_row; long long ys_ch; int ys_row; int C; float R; int clamp; int vec_x; int vec_y; double iR;
};

__device__ __forceinline__ float clamp_r(float v, float R) { return fminf(fmaxf(v, 0.f), R); }

// four pixels from p, the first nv (1 .. 4) of them inside the image, 0 for the others
__device__ __forceinline__ void load4(const float* __restrict__ p, int nv, bool vec, float (&f)[4]) {
  if (vec && nv == 4) {
    const F4 t = *reinterpret_cast<const F4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = t.f[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = k < nv ? p[k] : 0.f;
  }
}

// the luminance / R of the four pixels of one image row from column c0 (c0 % 4 == 0, c0 < W), 0 beyond the image
template <bool IS_X>
__device__ __forceinline__ void row_lum(const Src& s, int W, int row, int c0, double (&l)[4]) {
  const int nv = W - c0 < 4 ? W - c0 : 4;
  const float* const p = IS_X ? s.x + (long long)row * s.xs_row + c0 : s.y + (long long)row * s.ys_row + c0;
  const long long chs = IS_X ? s.xs_ch : s.ys_ch;
  const bool vec = IS_X ? s.vec_x != 0 : s.vec_y != 0;
  const bool cl = IS_X && s.clamp;
  float a[4];
  load4(p, nv, vec, a);
  if (cl) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = clamp_r(a[k], s.R);
  }
  if (s.C == 3) {
    float g[4], b[4];
    load4(p + chs, nv, vec, g);
    load4(p + 2 * chs, nv, vec, b);
    if (cl) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { g[k] = clamp_r(g[k], s.R); b[k] = clamp_r(b[k], s.R); }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) l[k] = ((0.299 * (double)a[k] + 0.587 * (double)g[k]) + 0.114 * (double)b[k]) * s.iR;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) l[k] = (double)a[k] * s.iR;
  }
}

// u (IS_X) or v of the cells (py, px) and (py, px + 1), px even: ((p00 + p01) + (p10 + p11)) * 0.25, 0 outside the map
template <bool IS_X>
__device__ __forceinline__ void cell_pair(const Src& s, int H, int W, int hp, int wp, int py, int px, double& c0v, double& c1v) {
  c0v = 0.0; c1v = 0.0;
  if (py < 0 || py >= hp || px < 0 || px >= wp) return;      // (px is even: with px outside the map px + 1 is outside too)
  double top[4], bot[4] = {0.0, 0.0, 0.0, 0.0};
  row_lum<IS_X>(s, W, 2 * py, 2 * px, top);                  // 2 py < H and 2 px < W follow from py < hp, px < wp
  if (2 * py + 1 < H) row_lum<IS_X>(s, W, 2 * py + 1, 2 * px, bot);
  c0v = ((top[0] + top[1]) + (bot[0] + bot[1])) * 0.25;
  c1v = ((top[2] + top[3]) + (bot[2] + bot[3])) * 0.25;      // (a cell beyond wp has only pixels beyond W: 0)
}

// U, V [TP + 2 HY][LW]: the cells (py0 - HY + r, px0 - HX + c)
template <int HY>
__device__ __forceinline__ void stage(double* __restrict__ U, double* __restrict__ V, const Src& s, int H, int W, int hp, int wp, int py0,
                                      int px0) {
  constexpr int ROWS = TP + 2 * HY, PAIRS = LW / 2;
  for (int it = threadIdx.x; it < ROWS * PAIRS; it += NT) {
    const int r = it / PAIRS, j = it - r * PAIRS;
    const int py = py0 - HY + r, px = px0 - HX + 2 * j;
    double a0, a1, b0, b1;
    cell_pair<true>(s, H, W, hp, wp, py, px, a0, a1);
    cell_pair<false>(s, H, W, hp, wp, py, px, b0, b1);
    U[r * LW + 2 * j] = a0; U[r * LW + 2 * j + 1] = a1;
    V[r * LW + 2 * j] = b0; V[r * LW + 2 * j + 1] = b1;
  }
}

// the Prewitt pair at LDS position (r, c), differences first: a flat neighbourhood gives exactly 0
__device__ __forceinline__ void prewitt(const double* __restrict__ P, int r, int c, double& gx, double& gy) {
  const double* const a = P + (r - 1) * LW + c;
  const double* const b = a + LW;
  const double* const d = b + LW;
  gx = ((a[1] - a[-1]) + (b[1] - b[-1]) + (d[1] - d[-1])) / 3.0;
  gy = ((d[-1] - a[-1]) + (d[0] - a[0]) + (d[1] - a[1])) / 3.0;
}

struct Entry { double gx, gy, m, mp, D, d; };

__device__ __forceinline__ Entry entry(const double* __restrict__ U, const double* __restrict__ V, int r, int c) {
  Entry e;
  double hx, hy;
  prewitt(U, r, c, e.gx, e.gy);
  prewitt(V, r, c, hx, hy);
  e.m = sqrt(e.gx * e.gx + e.gy * e.gy);
  e.mp = sqrt(hx * hx + hy * hy);
  e.D = e.m * e.m + e.mp * e.mp + T;
  const double df = e.m - e.mp;
  e.d = df * df / e.D;
  return e;
}

// Phase 1: the sums of d and d^2 over the tile's cells inside the map, to every thread.
__device__ __forceinline__ void value_tile(unsigned char* smem, const Src& s, int H, int W, int hp, int wp, int py0, int px0, double& sd,
                                           double& sd2) {
  double* const red = (double*)smem;
  double* const U = (double*)(smem + RED_BYTES);
  double* const V = U + (TP + 2) * LW;
  stage<1>(U, V, s, H, W, hp, wp, py0, px0);
  __syncthreads();
  double a = 0.0, q = 0.0;
  for (int it = threadIdx.x; it < TP * TP; it += NT) {
    const int ty = it / TP, tx = it - ty * TP;
    if (py0 + ty >= hp || px0 + tx >= wp) continue;
    const Entry e = entry(U, V, ty + 1, tx + HX);
    a += e.d;
    q += e.d * e.d;
  }
  sd = block_sum<NT>(a, red);
  sd2 = block_sum<NT>(q, red);
}

// the transposed Prewitt pair at position (r, c) of the (a_x, a_y) region
__device__ __forceinline__ double prewitt_adjoint(const double* __restrict__ AX, const double* __restrict__ AY, int r, int c) {
  const double* const xa = AX + (r - 1) * AW + c;
  const double* const xb = xa + AW;
  const double* const xd = xb + AW;
  const double* const ya = AY + (r - 1) * AW + c;
  const double* const yd = ya + 2 * AW;
  const double fx = ((xa[-1] - xa[1]) + (xb[-1] - xb[1]) + (xd[-1] - xd[1])) / 3.0;
  const double fy = ((ya[-1] - yd[-1]) + (ya[0] - yd[0]) + (ya[1] - yd[1])) / 3.0;
  return fx + fy;
}

// Phase 2: gx[q] += (float)(0.25 w_ch / R * dGMSD/du(cell of q) * coef ...) for the pixels of the tile; coef = scale / (n GMSD_b),
// mean_d = sum d / n (s_i - mu = mean_d - d_i).
__device__ __forceinline__ void grad_tile(unsigned char* smem, const Src& s, int H, int W, int hp, int wp, int py0, int px0, double coef,
                                          double mean_d, float* __restrict__ gx) {
  double* const U = (double*)(smem + RED_BYTES);
  double* const V = U + (TP + 4) * LW;
  double* const AX = V + (TP + 4) * LW;
  double* const AY = AX + AW * AW;
  stage<2>(U, V, s, H, W, hp, wp, py0, px0);
  __syncthreads();
  for (int it = threadIdx.x; it < AW * AW; it += NT) {
    const int r = it / AW, c = it - r * AW;
    const int py = py0 - 1 + r, px = px0 - 1 + c;
    double ax = 0.0, ay = 0.0;
    if (py >= 0 && py < hp && px >= 0 && px < wp) {
      const Entry e = entry(U, V, r + 1, c + 1);
      if (e.m > 0.0) {                                        // m = 0: gx = gy = 0, the entry adds nothing (no 0 * inf)
        const double rho = e.mp / e.m;
        const double sv = (2.0 * e.m * e.mp + T) / e.D;
        const double a = coef * (mean_d - e.d) * (2.0 * (rho - sv) / e.D);
        ax = a * e.gx;
        ay = a * e.gy;
      }
    }
    AX[it] = ax;
    AY[it] = ay;
  }
  __syncthreads();
  const double k = 0.25 * s.iR;
  for (int it = threadIdx.x; it < TP * TP / 2; it += NT) {
    const int ty = it / (TP / 2), pc = it - ty * (TP / 2);
    const int py = py0 + ty, px = px0 + 2 * pc;
    if (py >= hp || px >= wp) continue;
    double du[2];
    du[0] = prewitt_adjoint(AX, AY, ty + 1, 2 * pc + 1);
    du[1] = px + 1 < wp ? prewitt_adjoint(AX, AY, ty + 1, 2 * pc + 2) : 0.0;
    const int c0 = 2 * px;
    const int nv = W - c0 < 4 ? W - c0 : 4;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int row = 2 * py + dy;
      if (row >= H) break;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (ch >= s.C) break;
        const double wk = (s.C == 3 ? (ch == 0 ? 0.299 : ch == 1 ? 0.587 : 0.114) : 1.0) * k;
        const long long o = (long long)ch * s.xs_ch + (long long)row * s.xs_row + c0;
        if (s.vec_x && nv == 4) {
          const F4 xv = *reinterpret_cast<const F4*>(s.x + o);
          F4 g = *reinterpret_cast<const F4*>(gx + o);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (s.clamp && !(xv.f[q] >= 0.f && xv.f[q] <= s.R)) continue;         // the clamp passes no gradient
            g.f[q] = g.f[q] + (float)(wk * du[q >> 1]);                           // one fp32 rounding, one fp32 add per element
          }
          *reinterpret_cast<F4*>(gx + o) = g;
        } else {
          for (int q = 0; q < nv; ++q) {
            const float xv = s.x[o + q];
            if (s.clamp && !(xv >= 0.f && xv <= s.R)) continue;
            gx[o + q] = gx[o + q] + (float)(wk * du[q >> 1]);
          }
        }
      }
    }
  }
}

}  // namespace gmsd_tile
#endif
