// m2t_jpeg_tile.h -- the device text of k_jpeg.hip (include/m2t_jpeg.h): one workgroup takes the 8-bit values of one 16 x 16 tile of one
// item -- exactly 2 x 2 JPEG blocks, the tile grid and the block grid both start at the item's origin -- through the colour transform,
// the 8 x 8 DCT, the quantiser of the item's quality and the way back, one output per thread per plane and pass.  The values come
// from run_tile of m2t_degrade_tile.h (a store functor puts them into LDS as Y / Cb / Cr - 128) or straight from a uint8 image.
// Plain C++ on purpose: tests/jpeg_emulate.cpp runs this text on host threads (tests/emulate_hip).  fp64 multiplies and adds are
// SEPARATE roundings (-ffp-contract=off, build.FLAGS); there is no fp64 division and no transcendental here: T and recip come in
// from the host.
//
// LDS: T with rows of 9 doubles (the eight rows a 32-lane half reads start 18 dwords apart: eight distinct bank pairs of the 64 that
// a 64-bit read sees; equal addresses broadcast), the planes with rows of 17 doubles (a transposed sample walks a column of the tile:
// sixteen rows 34 dwords apart are sixteen distinct bank pairs).  The second plane buffer of the degrade kernels lies over the HR halo
// tile, which is dead once every thread has stored its pixel.
#pragma once
#include "m2t_degrade_tile.h"

namespace jpeg_tile {

using degrade_tile::CH;
using degrade_tile::NT;
using degrade_tile::TL;

constexpr int TP = 9;                   // doubles per row of T in LDS
constexpr int PP = 17;                  // doubles per row of a plane in LDS
constexpr int PLANE = TL * PP;
constexpr int WORK_DOUBLES = CH * PLANE;
constexpr int N_CONSTS = 64 + 256;      // T[8][8], recip[256]

struct JSmem {
  double T[8 * TP];
  double a[CH * PLANE];                 // f = plane - 128, then the dequantised coefficients
};
static_assert(sizeof(double) * WORK_DOUBLES <= degrade_tile::TILE_BYTES, "the second plane buffer lies over the halo tile");
static_assert(sizeof(degrade_tile::Smem::w) % sizeof(double) == 0, "the halo tile starts on a double");

// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
constexpr int BASE[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// S of a quality 1 .. 100, and entry k (natural order) of the luminance (chroma = 0) or chrominance table: integers only
__host__ __device__ inline int quant_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
__host__ __device__ inline int quant_entry(int chroma, int k, int S) {
  const int v = (BASE[chroma][k] * S + 50) / 100;
  return v < 1 ? 1 : v > 255 ? 255 : v;
}

__device__ __forceinline__ double level(double v) { return fmin(fmax(rint(v), 0.0), 255.0); }

// The pixel (py, px) of the tile: R, G, B -> Y, Cb, Cr - 128 into the planes
__device__ __forceinline__ void put_ycc(JSmem& js, int py, int px, const int (&q)[CH]) {
  const double r = (double)q[0], g = (double)q[1], b = (double)q[2];
  const double y = level((0.299 * r + 0.587 * g) + 0.114 * b);
  const double cb = level(((128.0 - 0.168736 * r) - 0.331264 * g) + 0.5 * b);
  const double cr = level(((128.0 + 0.5 * r) - 0.418688 * g) - 0.081312 * b);
  double* dst = js.a + py * PP + px;
  dst[0] = y - 128.0; dst[PLANE] = cb - 128.0; dst[2 * PLANE] = cr - 128.0;
}

struct PutYcc {                         // the store functor handed to run_tile
  JSmem* js; int ty0, tx0;
  __device__ __forceinline__ void operator()(int y, int x, const int (&q)[CH]) const { put_ycc(*js, y - ty0, x - tx0, q); }
};

// The stage over the tile whose rows x cols pixels lie in js.a (put_ycc; no barrier needed before the call).  `work` holds WORK_DOUBLES
// doubles of LDS that nobody reads after the call's first barrier.  `swap` as in run_tile; store(y, x, q) receives the pixel's position
// inside the item.  A block without a pixel inside the item is skipped by its 64 threads; the barriers are reached by every thread.
template <class Store>
__device__ __forceinline__ void stage(JSmem& js, double* work, const double* consts, int quality, int rows, int cols, int ty0, int tx0,
                                      bool swap, Store store) {
  const int t = threadIdx.x;
  if (t < 64) js.T[(t >> 3) * TP + (t & 7)] = consts[t];
  __syncthreads();
  const int a = t / TL, b = t - a * TL;
  const int py = swap ? b : a, px = swap ? a : b;
  const int y0 = py & ~7, x0 = px & ~7, i = py & 7, j = px & 7;          // the block's corner in the tile, the position in the block
  const bool present = y0 < rows && x0 < cols;
  const int S = quant_scale(quality);
  const int at = py * PP + px;
  if (present) {                                                          // g[i][v] = sum_j T[v][j] f[i][j], v = j of this thread
    const int sy = py < rows ? py : rows - 1;
    const double* tv = js.T + j * TP;
    for (int c = 0; c < CH; ++c) {
      const double* f = js.a + c * PLANE + sy * PP;
      double acc = 0.0;
      for (int k = 0; k < 8; ++k) acc = acc + tv[k] * f[x0 + k < cols ? x0 + k : cols - 1];
      work[c * PLANE + at] = acc;
    }
  }
  __syncthreads();
  if (present) {                                                          // F[u][v] = sum_i T[u][i] g[i][v], (u, v) = (i, j); quantise
    const double* tu = js.T + i * TP;
    for (int c = 0; c < CH; ++c) {
      const double* g = work + c * PLANE + y0 * PP + px;
      double acc = 0.0;
      for (int k = 0; k < 8; ++k) acc = acc + tu[k] * g[k * PP];
      const int Q = quant_entry(c != 0, i * 8 + j, S);
      const double coef = rint(acc * consts[64 + Q]);
      js.a[c * PLANE + at] = coef * (double)Q;
    }
  }
  __syncthreads();
  if (present) {                                                          // h[i][v] = sum_u T[u][i] d[u][v]
    for (int c = 0; c < CH; ++c) {
      const double* d = js.a + c * PLANE + y0 * PP + px;
      double acc = 0.0;
      for (int k = 0; k < 8; ++k) acc = acc + js.T[k * TP + i] * d[k * PP];
      work[c * PLANE + at] = acc;
    }
  }
  __syncthreads();
  if (py < rows && px < cols) {                                           // o[i][j] = sum_v T[v][j] h[i][v]; back to R, G, B
    double p[CH];
    for (int c = 0; c < CH; ++c) {
      const double* h = work + c * PLANE + py * PP + x0;
      double acc = 0.0;
      for (int k = 0; k < 8; ++k) acc = acc + js.T[k * TP + j] * h[k];
      p[c] = level(acc + 128.0);
    }
    const double cb = p[1] - 128.0, cr = p[2] - 128.0;
    int q[CH];
    q[0] = (int)level(p[0] + 1.402 * cr);
    q[1] = (int)level((p[0] - 0.344136 * cb) - 0.714136 * cr);
    q[2] = (int)level(p[0] + 1.772 * cb);
    store(ty0 + py, tx0 + px, q);
  }
}

// run_tile of m2t_degrade_tile.h followed by the stage; quality 0 is run_tile itself.  quality is the same for the whole workgroup.
template <class Store>
__device__ __forceinline__ void run_degrade_jpeg_tile(degrade_tile::Smem& sm, JSmem& js, const degrade_tile::Item& it, const double* consts,
                                                      int quality, int ty0, int tx0, bool swap, Store store) {
  if (quality == 0) {
    degrade_tile::run_tile(sm, it, ty0, tx0, swap, store);
    return;
  }
  degrade_tile::run_tile(sm, it, ty0, tx0, swap, PutYcc{&js, ty0, tx0});
  const int rows = it.lh - ty0 < TL ? it.lh - ty0 : TL, cols = it.lw - tx0 < TL ? it.lw - tx0 : TL;
  stage(js, reinterpret_cast<double*>(sm.tile), consts, quality, rows, cols, ty0, tx0, swap, store);
}

// The stage alone on the tile (ty0, tx0) of a uint8 [lh][lw][CH] image
template <class Store>
__device__ __forceinline__ void run_image_tile(JSmem& js, double* work, const uint8_t* img, int lh, int lw, const double* consts, int quality,
                                               int ty0, int tx0, Store store) {
  const int rows = lh - ty0 < TL ? lh - ty0 : TL, cols = lw - tx0 < TL ? lw - tx0 : TL;
  const int py = threadIdx.x / TL, px = threadIdx.x - py * TL;
  if (py < rows && px < cols) {
    const uint8_t* src = img + ((long long)(ty0 + py) * lw + tx0 + px) * CH;
    const int q[CH] = {src[0], src[1], src[2]};
    put_ycc(js, py, px, q);
  }
  stage(js, work, consts, quality, rows, cols, ty0, tx0, false, store);
}

}  // namespace jpeg_tile
