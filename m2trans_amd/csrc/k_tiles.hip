// k_tiles.hip -- tiled inference (include/m2t_tiles.h): the grid of overlapping tiles (host), the gather of a chunk of LR tiles into a
// batch, and the feather blend of the tiles' outputs into one SR image with an optional seam map.
//
// Pure data movement, so the one thing to get right is that every global load and store runs along the fastest axis.
//   gather  a plain coalesced copy: a workgroup (64 lanes along x, 4 rows) owns a 64 x 16 block of one destination plane; tile origins
//           are unaligned, so the accesses are dwords.
//   blend   a workgroup (256 threads = 8 rows of 32 lanes) owns one 32 x 32 block of the C output planes of one image.  The first
//           wave forms, once and in fp64, the <= 3 (tile, weight) pairs of each of the block's 32 rows and 32 columns into LDS: the
//           only divisions of the kernel, and only where tiles overlap.  The pairs are the same for every plane, so the block walks
//           the C planes with them (a block per plane took 51 us where this takes 44 at [1,3,2048,2048] on an MI355X).  A pair is
//           stored as the part of the tile element's offset that its axis decides, so a pixel's address in tile (ky, kx) is
//           rowoff + coloff + the channel's plane.  Elements that one tile covers are copied, the loads of a thread's four rows in
//           flight together; for the others a thread walks its pixel's <= 9 pairs, ky outside and kx inside.  Consecutive lanes
//           read consecutive u of the same tile, except across a tile edge.
// LDS: per axis and pair slot m a row of 32 doubles / 32 offsets (structure of arrays).  Lane tx reads column entry tx: 32 consecutive
// 8-byte words are the 64 banks of ds_read_b64, once; the row entry is one address per 32-lane half, a broadcast.
// Edge blocks are predicated per element, offsets are 64-bit, no atomics (two runs are bit-identical), no scratch (the pair loops
// are unrolled 3 x 3 and predicated, so the nine values of a pixel sit in registers).
#include "m2t_common.h"
#include "../../include/m2t_tiles.h"
#include <math.h>

namespace {

constexpr int BLK = 32;                        // the blend's block side
constexpr int RPT = BLK / 8;                   // block rows per thread
constexpr int MAXC = 3;                        // tiles that can cover a pixel on one axis
constexpr int GX = 64, GY = 4, GROWS = 16;     // the gather's block: 64 x 4 threads, 16 rows
constexpr int MAX_SIDE = 16384, MAX_SR_SIDE = 65536, MAX_PLANES = 65535, MAX_SCALE = 8;
constexpr long long MAX_GATHER_PLANES = 1ll << 22;

// the grid of one axis (m2t_tiles.h): n tiles of length t, origin(k) = min(k S, last)
struct Axis {
  int L, S, n, t, last;
  __host__ __device__ int origin(int k) const {
    const int r = k * S;                       // (n - 1) S < L + S <= 32768
    return r < last ? r : last;
  }
};

Axis make_axis(int L, int T, int overlap) {
  Axis a;
  a.L = L;
  a.S = T - overlap;
  if (L <= T) {
    a.n = 1, a.t = L, a.last = 0;
  } else {
    a.n = ceil_div(L - T, a.S) + 1, a.t = T, a.last = L - T;
  }
  return a;
}

// grid.x = planes * xblocks with plane = (tile - first) * C + c, grid.y = blocks of 16 rows
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ src, int C, int H, int W, Axis ay, Axis ax, int first,
                                                          int xblocks, float* __restrict__ dst) {
  const int tx = threadIdx.x & (GX - 1), ty = threadIdx.x >> 6;
  const int plane = blockIdx.x / xblocks, xb = blockIdx.x - plane * xblocks;
  const int g = first + plane / C, c = plane % C;
  const int per = ay.n * ax.n;
  const int b = g / per, k = g - b * per;
  const int ky = k / ax.n, kx = k - ky * ax.n;
  const int th = ay.t, tw = ax.t;
  const float* s = src + (((long long)b * C + c) * H + ay.origin(ky)) * W + ax.origin(kx);
  float* d = dst + (long long)plane * th * tw;
  const int x = xb * GX + tx;
  if (x >= tw) return;
#pragma unroll
  for (int q = 0; q < GROWS / GY; ++q) {
    const int y = blockIdx.y * GROWS + ty + GY * q;
    if (y < th) d[(long long)y * tw + x] = s[(long long)y * W + x];
  }
}

// The pairs of SR coordinate p on one axis into slot column `e` of the LDS rows: cnt, w[m], off[m] = tile_stride * k + u * u_stride.
__host__ __device__ __forceinline__ void axis_pairs(const Axis& a, int s, int p, long long tile_stride, long long u_stride, int e, int* cnt,
                                           double (*w)[BLK], long long (*off)[BLK]) {
  if (p >= s * a.L) {
    cnt[e] = 0;
    return;
  }
  const int q = p / s;
  const int k_hi = q >= a.last ? a.n - 1 : q / a.S;
  int k_lo = k_hi;
  while (k_lo > 0 && k_hi - k_lo < MAXC - 1 && a.origin(k_lo - 1) + a.t > q) --k_lo;
  cnt[e] = k_hi - k_lo + 1;
  const int st = s * a.t;
  for (int m = 0; m <= k_hi - k_lo; ++m) {
    const int k = k_lo + m, o = a.origin(k);
    const int u = p - s * o;
    const int fa = k >= 1 ? s * (a.origin(k - 1) + a.t - o) : 0;
    const int fb = k <= a.n - 2 ? s * (o + a.t - a.origin(k + 1)) : 0;
    double wt = 1.0;                           // a coordinate that one tile covers lies in neither ramp: both quotients exceed 1
    if (k_hi > k_lo && fa > 0) wt = fmin(wt, ((double)u + 0.5) / (double)fa);
    if (k_hi > k_lo && fb > 0) wt = fmin(wt, ((double)(st - u) - 0.5) / (double)fb);
    w[m][e] = wt;
    off[m][e] = tile_stride * k + u_stride * u;
  }
}

// grid (blocks along s W, blocks along s H, B)
template <bool SEAM>
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int C, Axis ay, Axis ax, int s,
                                                         float* __restrict__ dst, float* __restrict__ seam) {
  __shared__ double w[2][MAXC][BLK];           // [0] the rows' pairs, [1] the columns'
  __shared__ long long off[2][MAXC][BLK];
  __shared__ int cnt[2][BLK];
  const auto &wy = w[0], &wx = w[1];
  const auto &oy = off[0], &ox = off[1];
  const auto &cy = cnt[0], &cx = cnt[1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.y * BLK, j0 = blockIdx.x * BLK;
  const int Hs = s * ay.L, Ws = s * ax.L;
  const long long tplane = (long long)(s * ay.t) * (s * ax.t);     // one plane of one tile
  const int b = blockIdx.z;
  if (threadIdx.x < 2 * BLK) {                 // one wave, rows in its lower half and columns in its upper half, without divergence
    const bool col = threadIdx.x >= BLK;
    axis_pairs(col ? ax : ay, s, (col ? j0 : i0) + tx, col ? tplane * C : tplane * C * ax.n, col ? 1ll : (long long)s * ax.t, tx,
               cnt[col], w[col], off[col]);
  }
  __syncthreads();
  const int j = j0 + tx;
  const int nx = j < Ws ? cx[tx] : 0;
  // the pairs serve all C planes of the image: the block walks them
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    const float* z0 = tiles + ((long long)b * ay.n * ax.n * C + c) * tplane;
    const long long plane = (long long)b * C + c;
    // ---- elements that one tile covers: a copy; the loads of the thread's four rows are in flight together
    float v[RPT];
  #pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int r = ty + 8 * q;
      if (i0 + r < Hs && nx == 1 && cy[r] == 1) v[q] = z0[oy[0][r] + ox[0][tx]];
    }
  #pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int r = ty + 8 * q;
      if (i0 + r < Hs && nx == 1 && cy[r] == 1) {
        const long long o = (plane * Hs + i0 + r) * Ws + j;
        dst[o] = v[q];
        if constexpr (SEAM) seam[o] = 0.f;
      }
    }
    // ---- elements in an overlap: the <= 9 values of one element in registers
  #pragma unroll 1
    for (int q = 0; q < RPT; ++q) {
      const int r = ty + 8 * q, i = i0 + r;
      if (i >= Hs || j >= Ws) continue;
      const int ny = cy[r];
      if (ny * nx == 1) continue;
      const long long o = (plane * Hs + i) * Ws + j;
      float z[MAXC * MAXC];
      double wt[MAXC * MAXC];
  #pragma unroll
      for (int a = 0; a < MAXC; ++a)
  #pragma unroll
        for (int e = 0; e < MAXC; ++e)
          if (a < ny && e < nx) {
            z[a * MAXC + e] = z0[oy[a][r] + ox[e][tx]];
            wt[a * MAXC + e] = wy[a][r] * wx[e][tx];
          }
      double num = 0.0, den = 0.0;
  #pragma unroll
      for (int a = 0; a < MAXC; ++a)
  #pragma unroll
        for (int e = 0; e < MAXC; ++e)
          if (a < ny && e < nx) {
            num = num + wt[a * MAXC + e] * (double)z[a * MAXC + e];
            den = den + wt[a * MAXC + e];
          }
      const double m = num / den;
      dst[o] = (float)m;
      if constexpr (SEAM) {
        double acc = 0.0;
  #pragma unroll
        for (int a = 0; a < MAXC; ++a)
  #pragma unroll
          for (int e = 0; e < MAXC; ++e)
            if (a < ny && e < nx) {
              const double d = (double)z[a * MAXC + e] - m;
              acc = acc + wt[a * MAXC + e] * (d * d);
            }
        seam[o] = __fsqrt_rn((float)(acc / den));
      }
    }
  }
}

const char* grid_args(int L, int T, int overlap) {
  if (L < 1 || L > MAX_SIDE) return "the image side must be 1 .. 16384";
  if (T < 1 || T > MAX_SIDE) return "the tile size must be 1 .. 16384";
  if (overlap < 0 || 2 * overlap > T) return "the overlap must satisfy 0 <= 2 overlap <= tile size";
  return nullptr;
}

const char* batch_args(int B, int C) {
  if (B < 1 || C < 1 || (long long)B * C > MAX_PLANES) return "B C must be 1 .. 65535";
  return nullptr;
}

}  // namespace

extern "C" int m2t_tile_grid(int L, int T, int overlap, int* n_out, int* tile_len_out, int* origins_out) {
  const char* bad = !n_out || !tile_len_out ? "null pointer" : grid_args(L, T, overlap);
  if (bad) return m2t_set_error_at(M2T_ERR_ARG, "m2t_tile_grid", bad);
  const Axis a = make_axis(L, T, overlap);
  *n_out = a.n;
  *tile_len_out = a.t;
  if (origins_out)
    for (int k = 0; k < a.n; ++k) origins_out[k] = a.origin(k);
  return 0;
}

extern "C" int m2t_tile_gather(const float* src, int B, int C, int H, int W, int T, int overlap, int first, int count, float* dst,
                               void* stream) {
  const char* bad = nullptr;
  if (!src || !dst) bad = "null pointer";
  else if ((bad = grid_args(H, T, overlap)) || (bad = grid_args(W, T, overlap)) || (bad = batch_args(B, C))) {}
  else if (first < 0 || count < 1) bad = "first must be >= 0 and count >= 1";
  if (bad) return m2t_set_error_at(M2T_ERR_ARG, "m2t_tile_gather", bad);
  const Axis ay = make_axis(H, T, overlap), ax = make_axis(W, T, overlap);
  if ((long long)first + count > (long long)B * ay.n * ax.n)
    return m2t_set_error_at(M2T_ERR_ARG, "m2t_tile_gather", "first + count exceeds the tile count B ny nx");
  if ((long long)count * C > MAX_GATHER_PLANES)
    return m2t_set_error_at(M2T_ERR_ARG, "m2t_tile_gather", "count C must not exceed 2^22 (gather in chunks)");
  const int xblocks = ceil_div(ax.t, GX);      // <= 256, so grid.x <= 2^30
  const dim3 grid(count * C * xblocks, ceil_div(ay.t, GROWS), 1);
  tile_gather_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(src, C, H, W, ay, ax, first, xblocks, dst);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" int m2t_tile_blend(const float* tiles, int B, int C, int H, int W, int T, int overlap, int scale, float* dst, float* seam,
                              void* stream) {
  const char* bad = nullptr;
  if (!tiles || !dst) bad = "null pointer";
  else if ((bad = grid_args(H, T, overlap)) || (bad = grid_args(W, T, overlap)) || (bad = batch_args(B, C))) {}
  else if (scale < 1 || scale > MAX_SCALE) bad = "scale must be 1 .. 8";
  else if (scale * H > MAX_SR_SIDE || scale * W > MAX_SR_SIDE) bad = "s H and s W must not exceed 65536";
  if (bad) return m2t_set_error_at(M2T_ERR_ARG, "m2t_tile_blend", bad);
  const Axis ay = make_axis(H, T, overlap), ax = make_axis(W, T, overlap);
  const dim3 grid(ceil_div(scale * W, BLK), ceil_div(scale * H, BLK), B);
  if (seam) tile_blend_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(tiles, C, ay, ax, scale, dst, seam);
  else tile_blend_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(tiles, C, ay, ax, scale, dst, nullptr);
  M2T_LAUNCH_CHECK();
  return 0;
}
