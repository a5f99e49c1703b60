// m2t_wavelet_tile.h -- the tile text of the wavelet-domain loss term (k_wavelet_loss.hip; include/m2t_wavelet.h has the definition).
// It sits in a header so that tests/wavelet_emulate.cpp runs the same text on host threads.
//
// One level of the undecimated (a-trous) transform of ONE plane (an image's channel) per launch.  A workgroup of 256 threads owns a
// tile of TH x TW = 32 x 32 coefficients; the borders are periodic, so a tile at the edge stages wrapped rows and columns.  Everything
// behind the fp32 pixels is fp64; every tap sum runs k ascending from 0.0 with separate multiply and add.
//
//   stage      rows [r0, r0 + nrows) x columns [c0, c0 + ncols4) of the source, wrapped, into IN.  The work item is four columns of one
//              row: 16-byte loads where the alignment allows and the four do not cross the wrap, guarded scalar loads elsewhere.
//              The source is the difference d = c(x) / R - y / R formed from the fp32 pixels (level 1) or an fp64 plane (a_{j-1},
//              abar_j, psi).
//   fwd_tile   the tile plus (L - 1) s rows and columns below / right of it -> row pass with lo and hi into RL, RH -> column pass: the
//              four coefficients LH, HL, HH, LL of every pixel of the tile; four adjacent pixels of a row per thread.  Written as
//              asked: fp32 bands (the transform alone), w rho'(c) planes and the tile's sums of rho(c) (the loss), LL as the next
//              level's input.  A band of weight 0 costs neither rho nor a store.
//   bwd_tile   the adjoint of one level: per source plane present (abar_j, psi_LH | psi_HL, psi_HH) the tile plus (L - 1) s rows
//              above and halA columns left of it -> transposed column pass into RL | RH (the second plane of a pair is ADDED to the
//              first's result) -> transposed row pass, rl's sum plus rh's sum -> abar_{j-1} as an fp64 plane, or at level 1 the add
//              into the gradient through the clamp mask with ONE fp32 rounding.  halA = (L - 1) s rounded up to 4 keeps the staged
//              groups aligned.  An absent plane (weight 0) is neither staged nor passed.
// Elements outside [H, W] are never read or written.
//
// LDS (static): 64 B of reduction space | lo, hi: 2 x 8 doubles | IN (32 + HM)^2 doubles | RL, RH (32 + HM) x 32 doubles each, for a
// reach of at most HM.  Two variants: HM = 12 (haar and 3 taps at every level, db2 up to level 3) 38 208 B, four workgroups per CU;
// HM = 28 (8 taps at level 3) 59 712 B, two.
#ifndef M2T_WAVELET_TILE_H
#define M2T_WAVELET_TILE_H
#include <hip/hip_runtime.h>
#include <math.h>
#include "m2t_moment_tile.h"    // block_sum

namespace wavelet_tile {

using moment_tile::block_sum;

constexpr int TW = 32, TH = 32;                // coefficients per tile edge
constexpr int NT = 256;                        // threads per workgroup
constexpr int MAXL = 8, MAXJ = 3;              // taps, levels
constexpr int MAXB = 3 * MAXJ + 1;             // bands
constexpr int HM_BIG = (MAXL - 1) << (MAXJ - 1);      // the longest reach of one pass: 28
constexpr int HM_SMALL = 12;                   // haar and 3 taps at every level, db2 up to level 3: four workgroups per CU
constexpr size_t RED_BYTES = 64, FILT_BYTES = 2 * MAXL * sizeof(double);
// the staged region of a tile for a reach of at most HM: two variants of every kernel, chosen per launch by the level's reach
template <int HM>
struct Geo {
  static constexpr int SW = TW + HM, SH = TH + HM;
  static constexpr size_t SMEM = RED_BYTES + FILT_BYTES + sizeof(double) * ((size_t)SH * SW + 2 * (size_t)SH * TW);
  static_assert(SH * TW >= TH * SW, "RL / RH hold [SH][TW] forward and [TH][SW] backward");
  static_assert(SW % 4 == 0 && HM % 4 == 0, "staged groups of four columns");
};
__host__ __device__ constexpr bool small_reach(int taps, int dil) { return (taps - 1) * dil <= HM_SMALL; }

struct alignas(16) F4 { float f[4]; };
struct alignas(16) D2 { double d[2]; };

struct Filt { double lo[MAXL], hi[MAXL]; int taps; };

// ONE plane of the pair: x with a row stride (optionally clamped to [0, R]), y contiguous (never clamped); y == nullptr: the
// transform of x itself (d = x).  vec_x / vec_y: every row starts on a 16-byte boundary (decided on the host).
struct Src { const float* x; const float* y; long long xs_ch; int xs_row; float R; int clamp; int vec_x; int vec_y; double iR; };

__device__ __forceinline__ int wrap(int v, int n) { v %= n; return v < 0 ? v + n : v; }
__device__ __forceinline__ float clamp_r(float v, float R) { return fminf(fmaxf(v, 0.f), R); }

__device__ __forceinline__ double diff(const Src& s, float xv, float yv) {
  if (!s.y) return (double)xv;
  if (s.clamp) xv = clamp_r(xv, s.R);
  return (double)xv * s.iR - (double)yv * s.iR;
}

// the difference plane as a source of stage()
struct DiffSource {
  Src s; int W;
  __device__ __forceinline__ double one(int r, int c) const {
    return diff(s, s.x[(long long)r * s.xs_row + c], s.y ? s.y[(long long)r * W + c] : 0.f);
  }
  __device__ __forceinline__ void four(int r, int c, double (&v)[4]) const {      // c + 4 <= W
    float a[4], b[4] = {0.f, 0.f, 0.f, 0.f};
    const float* const px = s.x + (long long)r * s.xs_row + c;
    if (s.vec_x && (c & 3) == 0) {
      const F4 t = *reinterpret_cast<const F4*>(px);
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = t.f[q];
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = px[q];
    }
    if (s.y) {
      const float* const py = s.y + (long long)r * W + c;
      if (s.vec_y && (c & 3) == 0) {
        const F4 t = *reinterpret_cast<const F4*>(py);
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = t.f[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = py[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = diff(s, a[q], b[q]);
  }
};

// an fp64 plane [H][W] as a source of stage(); vec: every row starts on a 16-byte boundary (W even, the base aligned)
struct PlaneSource {
  const double* p; int W; int vec;
  __device__ __forceinline__ double one(int r, int c) const { return p[(long long)r * W + c]; }
  __device__ __forceinline__ void four(int r, int c, double (&v)[4]) const {
    const double* const q = p + (long long)r * W + c;
    if (vec && (c & 1) == 0) {
      const D2 a = *reinterpret_cast<const D2*>(q), b = *reinterpret_cast<const D2*>(q + 2);
      v[0] = a.d[0]; v[1] = a.d[1]; v[2] = b.d[0]; v[3] = b.d[1];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = q[k];
    }
  }
};

// IN[r][c] = source[(r0 + r) mod H][(c0 + c) mod W] for r < nrows, c < ncols4 (a multiple of 4, <= SW)
template <int HM, class Source>
__device__ __forceinline__ void stage(double* __restrict__ IN, const Source& src, int H, int W, int r0, int c0, int nrows, int ncols4) {
  const int groups = ncols4 >> 2;
  for (int it = threadIdx.x; it < nrows * groups; it += NT) {
    const int r = it / groups, g = it - r * groups;
    const int gr = wrap(r0 + r, H), gc = wrap(c0 + 4 * g, W);
    double v[4];
    if (gc + 4 <= W) {
      src.four(gr, gc, v);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = src.one(gr, wrap(gc + q, W));
    }
    double* const d = IN + r * Geo<HM>::SW + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = v[q];
  }
}

struct Lds { double* red; double* FL; double* FH; double* IN; double* RL; double* RH; };

template <int HM>
__device__ __forceinline__ Lds carve(unsigned char* smem, const Filt& f) {
  Lds l;
  l.red = (double*)smem;
  l.FL = (double*)(smem + RED_BYTES);
  l.FH = l.FL + MAXL;
  l.IN = l.FH + MAXL;
  l.RL = l.IN + Geo<HM>::SH * Geo<HM>::SW;
  l.RH = l.RL + Geo<HM>::SH * TW;
#pragma unroll
  for (int k = 0; k < MAXL; ++k)                      // (static indices: the taps stay in the argument registers)
    if ((int)threadIdx.x == k) { l.FL[k] = f.lo[k]; l.FH[k] = f.hi[k]; }
  return l;
}

// what one forward level writes for this plane; the four coefficients are k = 0 LH, 1 HL, 2 HH, 3 LL
struct FwdOut {
  float* band[4];       // fp32 [H][W] of coefficient k, or nullptr
  double* psi[4];       // fp64 [H][W] of w_k rho'(c_k), or nullptr
  double w[4];          // > 0: the tile's sum of rho(c_k) is formed
  double* a_out;        // fp64 [H][W] of LL, the next level's input, or nullptr
  double eps;
  int vec_f, vec_d;     // the rows of the fp32 / fp64 destinations start on 16-byte boundaries
};

__device__ __forceinline__ double rho(double c, double eps) { return eps > 0.0 ? sqrt(c * c + eps * eps) : fabs(c); }
__device__ __forceinline__ double rho_prime(double c, double eps) {
  if (eps > 0.0) return c / sqrt(c * c + eps * eps);
  return c > 0.0 ? 1.0 : c < 0.0 ? -1.0 : 0.0;
}

__device__ __forceinline__ void store4(double* __restrict__ p, const double (&v)[4], int nv, bool vec) {
  if (vec && nv == 4) {
    D2 a, b;
    a.d[0] = v[0]; a.d[1] = v[1]; b.d[0] = v[2]; b.d[1] = v[3];
    *reinterpret_cast<D2*>(p) = a;
    *reinterpret_cast<D2*>(p + 2) = b;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < nv) p[q] = v[q];
  }
}

// One forward level on the tile at (y0, x0): dil = 2^(j-1).  sum[k] = the tile's sum of rho(c_k) where o.w[k] > 0 (to every thread).
template <int HM, class Source>
__device__ __forceinline__ void fwd_tile(unsigned char* smem, const Source& src, int H, int W, int y0, int x0, int dil, const Filt& f,
                                         const FwdOut& o, double (&sum)[4]) {
  constexpr int SW = Geo<HM>::SW;
  const Lds l = carve<HM>(smem, f);
  const int th = H - y0 < TH ? H - y0 : TH, tw = W - x0 < TW ? W - x0 : TW;
  const int taps = f.taps, hal = (taps - 1) * dil, nrows = th + hal;      // hal <= HM
  stage<HM>(l.IN, src, H, W, y0, x0, nrows, (tw + hal + 3) & ~3);
  __syncthreads();
  for (int it = threadIdx.x; it < nrows * tw; it += NT) {                  // the row pass
    const int r = it / tw, c = it - r * tw;
    const double* const p = l.IN + r * SW + c;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < taps; ++k) {
      const double v = p[k * dil];
      a = a + l.FL[k] * v;
      b = b + l.FH[k] * v;
    }
    l.RL[r * TW + c] = a;
    l.RH[r * TW + c] = b;
  }
  __syncthreads();
  const int i = threadIdx.x >> 3, c4 = (threadIdx.x & 7) << 2;             // the column pass: four pixels of row i from column c4
  const bool live = i < th && c4 < tw;
  const int nv = !live ? 0 : tw - c4 < 4 ? tw - c4 : 4;
  double c[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) c[k][q] = 0.0;
  if (live) {
    for (int k = 0; k < taps; ++k) {
      const double* const pl = l.RL + (i + k * dil) * TW + c4;
      const double* const ph = l.RH + (i + k * dil) * TW + c4;
      const double fl = l.FL[k], fh = l.FH[k];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nv) break;
        c[0][q] = c[0][q] + fh * pl[q];      // LH = hi_col(lo_row)
        c[1][q] = c[1][q] + fl * ph[q];      // HL = lo_col(hi_row)
        c[2][q] = c[2][q] + fh * ph[q];      // HH
        c[3][q] = c[3][q] + fl * pl[q];      // LL
      }
    }
  }
  const long long at = (long long)(y0 + i) * W + x0 + c4;
  const bool four = ((x0 + c4) & 3) == 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (o.band[k] && live) {
      float* const p = o.band[k] + at;
      if (o.vec_f && nv == 4 && four) {
        F4 t;
#pragma unroll
        for (int q = 0; q < 4; ++q) t.f[q] = (float)c[k][q];
        *reinterpret_cast<F4*>(p) = t;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < nv) p[q] = (float)c[k][q];
      }
    }
    sum[k] = 0.0;
    if (o.w[k] > 0.0) {                                                    // (uniform over the workgroup)
      double a = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nv) a += rho(c[k][q], o.eps);
      sum[k] = block_sum<NT>(a, l.red);
      if (o.psi[k] && live) {
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = o.w[k] * rho_prime(c[k][q], o.eps);
        store4(o.psi[k] + at, v, nv, o.vec_d != 0);
      }
    }
  }
  if (o.a_out && live) store4(o.a_out + at, c[3], nv, o.vec_d != 0);
}

// the planes one backward level reads (nullptr: absent, weight 0) and where its result goes
struct BwdIn { const double* abar; const double* lh; const double* hl; const double* hh; int vec; };
struct GradDst { const float* x; float* gx; int xs_row; float R; int clamp; int vec; double coef; };      // coef = scale / R

// DST[i][c] (=|+=) sum_k F[k] * plane[(y0 + i - k dil) mod H][(x0 - halA + c) mod W] for i < th, c < ncols
template <int HM>
__device__ __forceinline__ void col_adjoint(const Lds& l, const double* plane, int vec, const double* F, double* __restrict__ DST, bool first,
                                            int H, int W, int y0, int x0, int th, int ncols, int hal, int halA, int dil, int taps) {
  constexpr int SW = Geo<HM>::SW;
  const PlaneSource src{plane, W, vec};
  stage<HM>(l.IN, src, H, W, y0 - hal, x0 - halA, th + hal, (ncols + 3) & ~3);
  __syncthreads();
  for (int it = threadIdx.x; it < th * ncols; it += NT) {
    const int i = it / ncols, c = it - i * ncols;
    const double* const p = l.IN + (i + hal) * SW + c;
    double t = 0.0;
    for (int k = 0; k < taps; ++k) t = t + F[k] * p[-k * dil * SW];
    DST[i * SW + c] = first ? t : DST[i * SW + c] + t;
  }
  __syncthreads();
}

// One backward level on the tile at (y0, x0).  LAST: gx += (float)(coef * abar_0) through the clamp mask, a value of exactly 0 leaving
// the element's bits alone; otherwise a_out = abar_{j-1}.
template <bool LAST, int HM>
__device__ __forceinline__ void bwd_tile(unsigned char* smem, const BwdIn& in, int H, int W, int y0, int x0, int dil, const Filt& f,
                                         double* __restrict__ a_out, int vec_d, const GradDst& g) {
  constexpr int SW = Geo<HM>::SW;
  const Lds l = carve<HM>(smem, f);
  const int th = H - y0 < TH ? H - y0 : TH, tw = W - x0 < TW ? W - x0 : TW;
  const int taps = f.taps, hal = (taps - 1) * dil, halA = (hal + 3) & ~3, ncols = tw + halA;      // hal <= HM, so halA <= HM
  __syncthreads();                                                         // (the taps are in LDS)
  const bool has_l = in.abar || in.lh, has_h = in.hl || in.hh;
  if (in.abar) col_adjoint<HM>(l, in.abar, in.vec, l.FL, l.RL, true, H, W, y0, x0, th, ncols, hal, halA, dil, taps);
  if (in.lh) col_adjoint<HM>(l, in.lh, in.vec, l.FH, l.RL, !in.abar, H, W, y0, x0, th, ncols, hal, halA, dil, taps);
  if (in.hl) col_adjoint<HM>(l, in.hl, in.vec, l.FL, l.RH, true, H, W, y0, x0, th, ncols, hal, halA, dil, taps);
  if (in.hh) col_adjoint<HM>(l, in.hh, in.vec, l.FH, l.RH, !in.hl, H, W, y0, x0, th, ncols, hal, halA, dil, taps);
  const int i = threadIdx.x >> 3, c4 = (threadIdx.x & 7) << 2;
  if (!(i < th && c4 < tw)) return;                                        // (no barrier below)
  const int nv = tw - c4 < 4 ? tw - c4 : 4;
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = 0.0;
    if (q >= nv) continue;
    double a = 0.0, b = 0.0;
    if (has_l) {
      const double* const p = l.RL + i * SW + c4 + q + halA;
      for (int k = 0; k < taps; ++k) a = a + l.FL[k] * p[-k * dil];
    }
    if (has_h) {
      const double* const p = l.RH + i * SW + c4 + q + halA;
      for (int k = 0; k < taps; ++k) b = b + l.FH[k] * p[-k * dil];
    }
    v[q] = a + b;
  }
  if (!LAST) {
    store4(a_out + (long long)(y0 + i) * W + x0 + c4, v, nv, vec_d != 0);
    return;
  }
  const long long o = (long long)(y0 + i) * g.xs_row + x0 + c4;
  if (g.vec && nv == 4) {
    const F4 xv = *reinterpret_cast<const F4*>(g.x + o);
    F4 t = *reinterpret_cast<const F4*>(g.gx + o);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (g.clamp && !(xv.f[q] >= 0.f && xv.f[q] <= g.R)) continue;        // the clamp passes no gradient
      const double d = g.coef * v[q];
      if (d != 0.0) t.f[q] = t.f[q] + (float)d;                            // one fp32 rounding, one fp32 add per element
    }
    *reinterpret_cast<F4*>(g.gx + o) = t;
  } else {
    for (int q = 0; q < nv; ++q) {
      const float xv = g.x[o + q];
      if (g.clamp && !(xv >= 0.f && xv <= g.R)) continue;
      const double d = g.coef * v[q];
      if (d != 0.0) g.gx[o + q] = g.gx[o + q] + (float)d;
    }
  }
}

}  // namespace wavelet_tile
#endif
