// m2t_degrade_tile.h -- the device text of k_degrade.hip (include/m2t_degrade.h): one workgroup turns one 16 x 16 tile of LR pixels
// of one item into 8-bit values: the HR halo tile and the item's K x K weights go to LDS, every thread walks the K x K taps of its own
// pixel in a fixed order (rows outer, columns inner, from 0.0) into three fp64 accumulators, adds the speckle and the additive noise of
// a counter-based generator and quantises.  Plain C++ on purpose: tests/degrade_emulate.cpp runs this text on host threads
// (tests/emulate_hip).  fp64 multiplies and adds are SEPARATE roundings: the library is built with -ffp-contract=off (build.FLAGS),
// and so is the emulator; a fused multiply-add here would change the bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace degrade_tile {

constexpr int TL = 16;                  // LR tile side
constexpr int NT = TL * TL;             // threads of a workgroup, one per LR pixel of the tile
constexpr int CH = 3;                   // channels (uint8 HWC)
constexpr int KMAX = 21;                // odd scales 1 .. 21, even scales 2 .. 20
constexpr int SIDE_MAX = 80;            // (TL - 1) * s + K at its largest: s = 4, K = 20
constexpr int TILE_BYTES = SIDE_MAX * SIDE_MAX * CH;

struct Smem {
  double w[KMAX * KMAX];                // the item's kernel, row-major
  uint8_t tile[TILE_BYTES];             // the halo tile, [rows][cols][CH] with `cols` the staged width
};

struct Item {
  const uint8_t* hr;                    // the HR image, uint8 [H][W][CH]
  const double* w;                      // K * K weights of this item
  int H, W;                             // HR image size (the fold's N, per axis)
  int ly, lx;                           // LR corner of the item in LR-image coordinates
  int lh, lw;                           // LR size of the item (the noise counter's row length is lw)
  int K, s;
  double sigma_add, sigma_speckle;      // grey levels / dimensionless; exactly 0 skips the generator
  unsigned long long noise_id;
  unsigned int seed_lo, seed_hi;        // the Philox key
  int gray;                             // 1: one variate per pixel for all channels
};

// A tap outside the image is folded symmetrically (-1 -> 0, -2 -> 1, N -> N - 1), period 2N, as often as it takes.
__device__ __forceinline__ int fold(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

__device__ __forceinline__ void mulhilo(unsigned int a, unsigned int b, unsigned int& hi, unsigned int& lo) {
  const unsigned long long p = (unsigned long long)a * (unsigned long long)b;
  hi = (unsigned int)(p >> 32);
  lo = (unsigned int)p;
}

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1) -> c[4]
__device__ __forceinline__ void philox4x32_10(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
  for (int r = 0; r < 10; ++r) {
    unsigned int h0, l0, h1, l1;
    mulhilo(0xD2511F53u, c[0], h0, l0);
    mulhilo(0xCD9E8D57u, c[2], h1, l1);
    const unsigned int n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = l1; c[2] = n2; c[3] = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// One variate: the twelve words of the blocks j = 0, 1, 2 summed as integers, g = (2 S + 12 - 12 * 2^32) / 2^33: exact in fp64,
// unit variance, support +-6 (Irwin-Hall).
__device__ __forceinline__ double variate(const Item& it, unsigned int c0, int sel, int ch) {
  unsigned long long S = 0;
  for (int j = 0; j < 3; ++j) {
    unsigned int c[4] = {c0, (unsigned int)(3 * sel + j + 8 * ch), (unsigned int)it.noise_id, (unsigned int)(it.noise_id >> 32)};
    philox4x32_10(c, it.seed_lo, it.seed_hi);
    S += (unsigned long long)c[0] + c[1] + c[2] + c[3];
  }
  const long long n = (long long)(2 * S + 12) - (12LL << 32);
  return (double)n * (1.0 / 8589934592.0);
}

// acc[CH] of the LR pixel (y, x) of the item -> the three 8-bit values
__device__ __forceinline__ void noise_and_quantise(const Item& it, int y, int x, const double (&acc)[CH], int (&q)[CH]) {
  const unsigned int c0 = (unsigned int)y * (unsigned int)it.lw + (unsigned int)x;
  double gs = 0.0, ga = 0.0;
  for (int c = 0; c < CH; ++c) {
    const int ch = it.gray ? 0 : c;
    if (c == 0 || !it.gray) {
      if (it.sigma_speckle != 0.0) gs = variate(it, c0, 1, ch);
      if (it.sigma_add != 0.0) ga = variate(it, c0, 0, ch);
    }
    double v = acc[c];
    if (it.sigma_speckle != 0.0) {
      double t = it.sigma_speckle * gs;
      t = t * acc[c];
      v = acc[c] + t;
    }
    if (it.sigma_add != 0.0) {
      const double u = it.sigma_add * ga;
      v = v + u;
    }
    const double r = fmin(fmax(rint(v), 0.0), 255.0);
    q[c] = (int)r;
  }
}

// Output position of the source-orientation pixel (y, x) of an n x n patch under the flags of m2t_crop_patches
// (bit0 hflip, bit1 vflip, bit2 transpose, applied in that order): the inverse of its index walk.
__device__ __forceinline__ void flipped(int flags, int n, int y, int x, int& oy, int& ox) {
  if (flags & 1) x = n - 1 - x;
  if (flags & 2) y = n - 1 - y;
  if (flags & 4) { oy = x; ox = y; } else { oy = y; ox = x; }
}

// The tile whose first LR pixel is (ty0, tx0) inside the item.  `swap` lets consecutive threads walk down a column of the source, so
// that a transposed store runs along the fastest axis of the output; the values do not depend on it.  store(y, x, q) receives the
// pixel's position inside the item, source orientation.  Every thread of the workgroup must call this (it holds barriers).
template <class Store> __device__ __forceinline__ void run_tile(Smem& sm, const Item& it, int ty0, int tx0, bool swap, Store store) {
  const int t = threadIdx.x;
  const int K = it.K, s = it.s;
  const int rows = it.lh - ty0 < TL ? it.lh - ty0 : TL, cols = it.lw - tx0 < TL ? it.lw - tx0 : TL;
  const int th = (rows - 1) * s + K, tw = (cols - 1) * s + K;             // staged extent, <= SIDE_MAX
  const int y0 = s * (it.ly + ty0) + (s - K) / 2, x0 = s * (it.lx + tx0) + (s - K) / 2;   // (s - K) is even: exact
  for (int i = t; i < K * K; i += NT) sm.w[i] = it.w[i];
  for (int i = t; i < th * tw; i += NT) {
    const int r = i / tw, c = i - r * tw;
    const uint8_t* src = it.hr + ((long long)fold(y0 + r, it.H) * it.W + fold(x0 + c, it.W)) * CH;
    uint8_t* dst = sm.tile + i * CH;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  }
  __syncthreads();
  const int a = t / TL, b = t - a * TL;
  const int dy = swap ? b : a, dx = swap ? a : b;
  if (dy < rows && dx < cols) {
    double acc[CH] = {0.0, 0.0, 0.0};
    const uint8_t* base = sm.tile + (dy * s * tw + dx * s) * CH;
    for (int i = 0; i < K; ++i) {
      const uint8_t* row = base + i * tw * CH;
      const double* wr = sm.w + i * K;
      for (int j = 0; j < K; ++j) {
        const double wv = wr[j];
        acc[0] = acc[0] + wv * (double)row[j * CH + 0];
        acc[1] = acc[1] + wv * (double)row[j * CH + 1];
        acc[2] = acc[2] + wv * (double)row[j * CH + 2];
      }
    }
    int q[CH];
    noise_and_quantise(it, ty0 + dy, tx0 + dx, acc, q);
    store(ty0 + dy, tx0 + dx, q);
  }
}

}  // namespace degrade_tile
