// m2t_consistency_tile.h -- the tile text of the LR-consistency family (k_consistency.hip; include/m2t_consistency.h has the
// definition).  It sits in a header so that tests/consistency_emulate.cpp runs the same text on host threads.
//
// D is the "down" case of include/m2t_resize.h: per axis of length n = m s, LR cell i takes the SR samples j = i s + M0 + t,
// t = 0 .. NTAP-1, folded by mirror_idx(j, n); rows first, then columns, fp64 throughout.  The geometry is the one of k_resize.hip
// (8 / 11 / 16 taps from M0 = -3 / -4 / -6 down, s phases of 5 taps from M0 = -2 up; the normalised fp64 taps are computed on the host
// and travel in the kernel arguments), restated here because k_resize.hip keeps it private.
//
//   down_tile     one workgroup (256 threads) per tile of 16 x 32 LR cells: the SR tile with its mirrored halo goes into LDS once as
//                 fp32 (through the optional clamp); per strip of 8 cell rows the vertical pass into an fp64 strip and the horizontal
//                 pass out of it, one cell per thread; r = (D c(x) - y) / R (back-projection: (y - D c(x)) / R), rho and rho' in
//                 registers; rho' (or r) goes to the fp64 plane; returns the tile's sums {sum rho, sum |r|, max |r|, sum r^2}.
//   adjoint_tile  D^T in gather form, one workgroup per tile of 32 x 64 SR pixels: the g cells the tile's pixels receive from are
//                 staged in LDS as fp64; per axis a table lists, for every pixel row / column of the tile, the (cell, weight) pairs
//                 whose folded taps land on it -- the unfolded positions j = q + 2 n k and j = 2 n - 1 - q + 2 n k inside
//                 [M0, n - 1 - M0], k ascending, q's images first, then per position the cells in ascending order: at most 4 pairs
//                 for every n (the repeated reflections of a short axis included).  Horizontal pass into an fp64 strip, vertical pass
//                 out of it, then the clamp mask, ONE fp32 rounding and one read-add-write (or store) of the destination element.
//   update_tile   back-projection's update, one workgroup per 16 x 16 LR cells = (16 s)^2 SR pixels: the fp64 residual tile with its
//                 mirrored halo of 2 in LDS, U (s phases of 5 taps) rows first, then columns, and
//                 sr <- clamp(fp32(sr + beta R U(r)), 0, R) four pixels of a row at a time (16-byte accesses where every row of sr
//                 starts on a 16-byte boundary).
//   finish_tile   one workgroup: folds the tiles' sums in a fixed order into loss_out / stats_out.
// No atomics, every output element is written by exactly one thread, sums in a fixed order: two runs are bit-identical.
//
// LDS (x4, the largest): down 64 + 8 * 140 * 8 + 76 * 140 * 4 + (76 + 140) * 4 = 52 448 B; adjoint < 22 KB; update < 14 KB.
#ifndef M2T_CONSISTENCY_TILE_H
#define M2T_CONSISTENCY_TILE_H
#include <hip/hip_runtime.h>
#include <math.h>
#include "m2t_moment_tile.h"    // block_sum

namespace cons_tile {

using moment_tile::block_sum;

constexpr int NT = 256;                        // threads per workgroup
constexpr int MAX_TAPS = 20;                   // 16 (x4 down) / 4 phases x 5 (x4 up)
struct Taps { double w[MAX_TAPS]; };           // down: [tap]; up: [phase][tap]
constexpr size_t RED_BYTES = 64;

template <int S> struct Down {
  static constexpr int NTAP = S == 2 ? 8 : S == 3 ? 11 : 16;
  static constexpr int M0 = S == 2 ? -3 : S == 3 ? -4 : -6;
  static constexpr int TQH = 16, TQW = 32;     // LR cells per tile
  static constexpr int SRQ = 8;                // cell rows per strip (SRQ * TQW = NT: one cell per thread)
  static constexpr int IH = (TQH - 1) * S + NTAP, IW = (TQW - 1) * S + NTAP;
  static constexpr size_t SMEM = RED_BYTES + sizeof(double) * SRQ * IW + sizeof(float) * IH * IW + sizeof(int) * (IH + IW);
};
struct Up { static constexpr int NTAP = 5, M0 = -2, TQ = 16, IN = TQ + NTAP - 1; };
template <int S> struct Adj {
  static constexpr int TH = 32, TW = 64;       // SR pixels per tile
  static constexpr int MAXP = 4;               // (cell, weight) pairs per pixel row / column
  static constexpr int GH = (TH + Down<S>::NTAP - 2) / S + 2, GW = (TW + Down<S>::NTAP - 2) / S + 2;   // g cells staged, at most
  static constexpr size_t SMEM = sizeof(double) * (MAX_TAPS + GH * GW + GH * TW + (TH + TW) * MAXP) + sizeof(int) * (TH + TW) * (MAXP + 1);
};
template <int S> struct Upd {
  static constexpr int RH = Up::TQ * S;        // SR rows (and columns) per tile
  static constexpr size_t SMEM = sizeof(double) * (MAX_TAPS + Up::IN * Up::IN + RH * Up::IN);
};

struct alignas(16) F4 { float f[4]; };

// MATLAB's aux = [1:n, n:-1:1] on 0-based indices: period 2n, edge pixel repeated; any j (the halo may wrap a short axis often)
__device__ __forceinline__ int mirror_idx(int j, int n) {
  const int p = 2 * n;
  int m = j % p;
  if (m < 0) m += p;
  return m < p - 1 - m ? m : p - 1 - m;
}

__device__ __forceinline__ float clamp_r(float v, float R) { return fminf(fmaxf(v, 0.f), R); }

// the maximum of v over the N threads of a workgroup, to every thread (the shape of block_sum)
template <int N>
__device__ __forceinline__ double block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < N / 64; ++w) t = fmax(t, red[w]);
  return t;
}

// cubic convolution kernel, a = -0.5, and the normalised taps (host; the expression order is the one of resize.filter_taps)
inline double cubic(double x) {
  x = fabs(x);
  if (x <= 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
  if (x <= 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
  return 0.0;
}
inline Taps make_taps(int S, bool up) {
  const int nt = up ? 5 : (S == 2 ? 8 : S == 3 ? 11 : 16), m0 = up ? -2 : (S == 2 ? -3 : S == 3 ? -4 : -6);
  Taps tp;
  for (int i = 0; i < MAX_TAPS; ++i) tp.w[i] = 0.0;
  for (int p = 0; p < (up ? S : 1); ++p) {
    double* w = tp.w + p * nt;
    double sum = 0.0;
    for (int t = 0; t < nt; ++t) {
      const int m = m0 + t;
      if (up) w[t] = cubic((2 * p + 1 - S - 2 * S * m) / (2.0 * S));
      else w[t] = cubic((S - 1 - 2 * m) / (2.0 * S)) / S;
      sum += w[t];
    }
    for (int t = 0; t < nt; ++t) w[t] /= sum;
  }
  return tp;
}

// ---- D, the residual and its statistics ---------------------------------------------------------------------------------------------
// xp: the SR plane [H S][W S] with row stride xs_row; yp: the LR plane [H][W], contiguous; plane: fp64 [H][W], contiguous.
// (qy0, qx0): the tile's first cell.  back_project == 0: r = (D c(x) - y) / R and plane = rho'(r); != 0: r = (y - D c(x)) / R and
// plane = r.  sums = {sum rho(r), sum |r|, max |r|, sum r^2} over the tile's cells inside the plane, to every thread.
template <int S>
__device__ __forceinline__ void down_tile(unsigned char* smem, const float* __restrict__ xp, int xs_row, const float* __restrict__ yp,
                                          int H, int W, int qy0, int qx0, float R, int clamp, double iR, double eps, int back_project,
                                          const Taps& taps, double* __restrict__ plane, double (&sums)[4]) {
  using G = Down<S>;
  constexpr int NTAP = G::NTAP, IW = G::IW;
  double* const red = (double*)smem;
  double* const mid = (double*)(smem + RED_BYTES);
  float* const tile = (float*)(smem + RED_BYTES + sizeof(double) * G::SRQ * IW);
  int* const fold = (int*)(tile + G::IH * IW);             // the mirrored row (IH) and column (IW) of every tile row / column
  const int tid = threadIdx.x;
  const int Hs = H * S, Ws = W * S;
  const int nqy = H - qy0 < G::TQH ? H - qy0 : G::TQH, nqx = W - qx0 < G::TQW ? W - qx0 : G::TQW;      // cells of this tile
  const int ih = (nqy - 1) * S + NTAP, iw = (nqx - 1) * S + NTAP;                                      // the SR samples they read
  const int ys = qy0 * S + G::M0, xs = qx0 * S + G::M0;

  // (the folds once per tile row and column, not once per sample: an integer remainder each)
  for (int i = tid; i < G::IH + IW; i += NT) fold[i] = i < G::IH ? mirror_idx(ys + i, Hs) : mirror_idx(xs + i - G::IH, Ws);
  __syncthreads();
  // (STAGE_U loads in flight per thread before the first LDS write: a one-by-one loop waits out the memory latency 42 times at x4)
  constexpr int STAGE_U = 8, PER = (G::IH * IW + NT - 1) / NT;
  for (int b0 = 0; b0 < PER; b0 += STAGE_U) {
    float v[STAGE_U];
#pragma unroll
    for (int u = 0; u < STAGE_U; ++u) {
      const int i = tid + (b0 + u) * NT, r = i / IW, c = i - r * IW;
      v[u] = (i < G::IH * IW && r < ih && c < iw) ? xp[(long long)fold[r] * xs_row + fold[G::IH + c]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < STAGE_U; ++u) {
      const int i = tid + (b0 + u) * NT, r = i / IW, c = i - r * IW;
      if (i < G::IH * IW && r < ih && c < iw) tile[i] = clamp ? clamp_r(v[u], R) : v[u];
    }
  }
  __syncthreads();

  double s_rho = 0.0, s_abs = 0.0, s_max = 0.0, s_sq = 0.0;
  for (int s0 = 0; s0 < G::TQH; s0 += G::SRQ) {
    // vertical pass: tile rows -> fp64 strip
    for (int i = tid; i < G::SRQ * IW; i += NT) {
      const int qq = i / IW, c = i - qq * IW;
      if (s0 + qq < nqy && c < iw) {
        const float* const col = tile + (s0 + qq) * S * IW + c;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < NTAP; ++t) acc += taps.w[t] * (double)col[t * IW];
        mid[i] = acc;
      }
    }
    __syncthreads();
    // horizontal pass: one cell per thread
    {
      const int qq = tid / G::TQW, qc = tid - qq * G::TQW;
      if (s0 + qq < nqy && qc < nqx) {
        const double* const m = mid + qq * IW + qc * S;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < NTAP; ++t) acc += taps.w[t] * m[t];
        const long long q = (long long)(qy0 + s0 + qq) * W + (qx0 + qc);
        const double y = (double)yp[q];
        const double r = back_project ? (y - acc) * iR : (acc - y) * iR;
        const double a = fabs(r);
        double rho, drho;
        if (eps > 0.0) {
          rho = sqrt(r * r + eps * eps);
          drho = r / rho;
        } else {
          rho = a;
          drho = r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0);
        }
        plane[q] = back_project ? r : drho;
        s_rho += rho; s_abs += a; s_max = fmax(s_max, a); s_sq += r * r;
      }
    }
    __syncthreads();
  }
  sums[0] = block_sum<NT>(s_rho, red);
  sums[1] = block_sum<NT>(s_abs, red);
  sums[2] = block_max<NT>(s_max, red);
  sums[3] = block_sum<NT>(s_sq, red);
}

// ---- D^T, gather form -----------------------------------------------------------------------------------------------------------------
// the first and the last LR cell whose taps (direct or reflected) reach the SR samples q0 .. q0 + len - 1 of an axis of m cells
template <int S>
__device__ __forceinline__ void adj_window(int q0, int len, int m, int& ilo, int& ihi) {
  using G = Down<S>;
  const int lo = q0 - G::M0 - G::NTAP + 1, hi = (q0 + len - 1 - G::M0) / S;
  ilo = lo <= 0 ? 0 : (lo + S - 1) / S;
  ihi = hi < m - 1 ? hi : m - 1;
}

// the (cell - ilo, weight) pairs of SR sample q on an axis of n = m S samples, in the fixed order of the header comment; wl: the taps
template <int S>
__device__ __forceinline__ void adj_pairs(int q, int n, int m, int ilo, const double* wl, int* idx, double* w, int& cnt_out) {
  using G = Down<S>;
  constexpr int MAXP = Adj<S>::MAXP;
  int cnt = 0;
  for (int side = 0; side < 2; ++side) {
    const int b = side ? 2 * n - 1 - q : q;
    for (int j = b - 2 * n * ((b - G::M0) / (2 * n)); j <= n - 1 - G::M0; j += 2 * n) {     // (b - M0 > 0: the first image at or above M0)
      const int a = j - G::M0, lo = a - G::NTAP + 1;
      const int i0 = lo <= 0 ? 0 : (lo + S - 1) / S, i1 = a / S < m - 1 ? a / S : m - 1;
      for (int i = i0; i <= i1; ++i)
        if (cnt < MAXP) { idx[cnt] = i - ilo; w[cnt] = wl[a - i * S]; ++cnt; }
    }
  }
  cnt_out = cnt;
}

// gp: the g plane [H][W] (GT = double: the rho' plane of the loss; float: the input of m2t_imresize_adjoint_f32), contiguous.
// op: the destination [H S][W S] with row stride os_row; xp (or nullptr: no mask): x with row stride xs_row, mask [0 <= x <= R] when
// clamp.  op[q] = (accumulate ? op[q] : 0) + (float)(coef * (D^T g)(q)) for the tile's pixels inside the plane the mask lets through.
template <int S, typename GT>
__device__ __forceinline__ void adjoint_tile(unsigned char* smem, const GT* __restrict__ gp, int H, int W, int y0, int x0,
                                             const float* __restrict__ xp, int xs_row, float R, int clamp, double coef, const Taps& taps,
                                             float* __restrict__ op, int os_row, int accumulate) {
  using A = Adj<S>;
  constexpr int TH = A::TH, TW = A::TW, MAXP = A::MAXP, GW = A::GW;
  double* const wl = (double*)smem;
  double* const Gt = wl + MAX_TAPS;
  double* const Ht = Gt + A::GH * GW;
  double* const tw = Ht + A::GH * TW;                      // [TH + TW][MAXP]: rows, then columns
  int* const ti = (int*)(tw + (TH + TW) * MAXP);           // [TH + TW][MAXP]
  int* const tc = ti + (TH + TW) * MAXP;                   // [TH + TW]
  const int tid = threadIdx.x;
  const int Hs = H * S, Ws = W * S;
  const int nh = Hs - y0 < TH ? Hs - y0 : TH, nw = Ws - x0 < TW ? Ws - x0 : TW;
  int iy0, iy1, ix0, ix1;
  adj_window<S>(y0, nh, H, iy0, iy1);
  adj_window<S>(x0, nw, W, ix0, ix1);
  const int gh = iy1 - iy0 + 1, gw = ix1 - ix0 + 1;        // (at most GH, GW)

#pragma unroll
  for (int i = 0; i < MAX_TAPS; ++i)
    if (tid == i) wl[i] = taps.w[i];
  for (int i = tid; i < A::GH * GW; i += NT) {
    const int r = i / GW, c = i - r * GW;
    if (r < gh && c < gw) Gt[i] = (double)gp[(long long)(iy0 + r) * W + (ix0 + c)];
  }
  __syncthreads();
  if (tid < TH + TW) {
    const bool row = tid < TH;
    const int k = row ? tid : tid - TH;
    int cnt = 0;
    if (row ? k < nh : k < nw) {
      if (row) adj_pairs<S>(y0 + k, Hs, H, iy0, wl, ti + tid * MAXP, tw + tid * MAXP, cnt);
      else adj_pairs<S>(x0 + k, Ws, W, ix0, wl, ti + tid * MAXP, tw + tid * MAXP, cnt);
    }
    tc[tid] = cnt;
  }
  __syncthreads();
  // horizontal pass: staged g rows -> the tile's pixel columns
  for (int i = tid; i < A::GH * TW; i += NT) {
    const int r = i / TW, c = i - r * TW;
    if (r < gh && c < nw) {
      const int n = tc[TH + c];
      const int* const id = ti + (TH + c) * MAXP;
      const double* const wt = tw + (TH + c) * MAXP;
      double acc = 0.0;
      for (int p = 0; p < n; ++p) acc += wt[p] * Gt[r * GW + id[p]];
      Ht[i] = acc;
    }
  }
  __syncthreads();
  // vertical pass, mask, one rounding, one read-add-write
  for (int i = tid; i < TH * TW; i += NT) {
    const int r = i / TW, c = i - r * TW;
    if (r < nh && c < nw) {
      bool pass = true;
      if (xp && clamp) {
        const float xv = xp[(long long)(y0 + r) * xs_row + (x0 + c)];
        pass = xv >= 0.f && xv <= R;
      }
      if (pass) {
        const int n = tc[r];
        const int* const id = ti + r * MAXP;
        const double* const wt = tw + r * MAXP;
        double acc = 0.0;
        for (int p = 0; p < n; ++p) acc += wt[p] * Ht[id[p] * TW + c];
        float* const o = op + (long long)(y0 + r) * os_row + (x0 + c);
        const float v = (float)(coef * acc);
        *o = accumulate ? *o + v : v;
      }
    }
  }
}

// ---- back-projection's update -----------------------------------------------------------------------------------------------------------
// rp: the residual plane [H][W] fp64; sp: the SR plane [H S][W S], contiguous; (qy0, qx0): the tile's first LR cell; taps: the up-sampler's
// [S][5]; bR = beta * R; vec: every row of sp starts on a 16-byte boundary (W S % 4 == 0 and an aligned base).
template <int S>
__device__ __forceinline__ void update_tile(unsigned char* smem, const double* __restrict__ rp, float* __restrict__ sp, int H, int W,
                                            int qy0, int qx0, float R, double bR, int vec, const Taps& taps) {
  constexpr int TQ = Up::TQ, NTAP = Up::NTAP, IN = Up::IN, RH = Upd<S>::RH, NG = RH / 4;
  double* const wl = (double*)smem;
  double* const in = wl + MAX_TAPS;
  double* const mid = in + IN * IN;                         // [RH][IN]
  const int tid = threadIdx.x;
  const int Ws = W * S, Hs = H * S;
#pragma unroll
  for (int i = 0; i < MAX_TAPS; ++i)
    if (tid == i) wl[i] = taps.w[i];
  for (int i = tid; i < IN * IN; i += NT) {
    const int r = i / IN, c = i - r * IN;
    in[i] = rp[(long long)mirror_idx(qy0 + Up::M0 + r, H) * W + mirror_idx(qx0 + Up::M0 + c, W)];
  }
  __syncthreads();
  for (int i = tid; i < RH * IN; i += NT) {
    const int row = i / IN, c = i - row * IN;
    const int q = row / S, p = row - q * S;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < NTAP; ++t) acc += wl[p * NTAP + t] * in[(q + t) * IN + c];
    mid[i] = acc;
  }
  __syncthreads();
  for (int i = tid; i < RH * NG; i += NT) {
    const int row = i / NG, g = i - row * NG;
    const int oy = qy0 * S + row, ox = qx0 * S + 4 * g;
    if (oy >= Hs || ox >= Ws) continue;
    float* const o = sp + (long long)oy * Ws + ox;
    const int nv = Ws - ox < 4 ? Ws - ox : 4;
    float v[4];
    if (vec) {                                              // (Ws % 4 == 0: nv == 4)
      const F4 t = *reinterpret_cast<const F4*>(o);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = t.f[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = k < nv ? o[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = 4 * g + k, q = col / S, p = col - q * S;
      const double* const m = mid + row * IN + q;
      double acc = 0.0;
#pragma unroll
      for (int t = 0; t < NTAP; ++t) acc += wl[p * NTAP + t] * m[t];
      v[k] = clamp_r((float)((double)v[k] + bR * acc), R);
    }
    if (vec) {
      F4 t;
#pragma unroll
      for (int k = 0; k < 4; ++k) t.f[k] = v[k];
      *reinterpret_cast<F4*>(o) = t;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nv) o[k] = v[k];
    }
  }
}

// ---- the fold ---------------------------------------------------------------------------------------------------------------------------
// part [nt][4] = the tiles' sums in tile order; n = the number of LR elements.  loss_out (or nullptr): (accumulate ? loss_out : 0) +
// (float)(scale * sum rho); stats_out (or nullptr): {mean |r|, max |r|, mean r^2}.  red: 64 bytes of LDS.
__device__ __forceinline__ void finish_tile(double* red, const double* __restrict__ part, long long nt, double n, double scale,
                                            int accumulate, float* __restrict__ loss_out, double* __restrict__ stats_out) {
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  for (long long i = threadIdx.x; i < nt; i += NT) {
    a += part[4 * i]; b += part[4 * i + 1]; c = fmax(c, part[4 * i + 2]); d += part[4 * i + 3];
  }
  a = block_sum<NT>(a, red);
  b = block_sum<NT>(b, red);
  c = block_max<NT>(c, red);
  d = block_sum<NT>(d, red);
  if (threadIdx.x != 0) return;
  if (loss_out) loss_out[0] = (accumulate ? loss_out[0] : 0.f) + (float)(scale * a);
  if (stats_out) { stats_out[0] = b / n; stats_out[1] = c; stats_out[2] = d / n; }
}

}  // namespace cons_tile
#endif
