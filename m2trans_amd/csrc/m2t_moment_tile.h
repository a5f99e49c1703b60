// m2t_moment_tile.h -- the one tile behind the windowed-moment loss terms: SSIM and MS-SSIM (m2t_ssim_tile.h) and VIF (m2t_vif_tile.h).
//
// One workgroup owns a TS x TS tile of a plane pair (x, y) under a separable WIN-tap window.  TM = TS + WIN - 1 map entries per tile
// edge have windows that touch the tile, TI = TM + WIN - 1 input samples per edge feed them.
//
//   maps()   1. the TI x TI raw tiles of both planes into LDS through load(), 0 outside the plane;
//            2. vertical pass of u, v, uu, vv, uv (u = use(raw x), v = raw y), an fp64 fma chain in tap order;
//            3. horizontal pass to five moments per map entry, then map(): three coefficient maps into D (the caller writes 0
//               outside the map: the zero extension of the transposed filter) and the sums over the entries the tile OWNS, those
//               whose top-left pixel lies in the tile (local r >= WIN - 1 and cc >= WIN - 1);
//   grad()   4. transposed filter of the three coefficient maps, vertical, into T -- aliased on V, which maps() has freed;
//            5. transposed filter, horizontal, then epi() once per pixel of the tile inside the plane, by one thread.
//
// What a term adds is five functors at the call site (all inlined):
//   load(gy, gxx, Raw& a, Raw& b)                                     the two raw samples of an in-plane position
//   use(Raw a) -> double                                              raw x to u where a value is used (the raw one stays in LDS)
//   map(const double (&m)[5], valid, owned, double (&d)[3], double (&acc)[NSUM])
//                                                                     m = G*u, G*v, G*uu, G*vv, G*uv; valid: the entry is in the map
//   pass(Raw x_raw) -> bool                                           false: the pixel gets no gradient.  Asked BEFORE step 5 filters:
//                                                                     the branch keeps the filter's loads behind it, and the SSIM
//                                                                     kernels at 71 / 69 / 87 VGPRs (85 / 85 / 102 with the mask in epi)
//   epi(gy, gxx, a0, a1, a2, Raw x_raw, Raw y_raw)                    a_k = G^T * d[k] at the pixel
//
// LDS (bytes): V = 5 TM TI doubles, D = 3 TM TM doubles, 8 doubles (or one per wave) of reduction space, the raw x | y tiles.
// Everything between the raw samples and the epilogue is fp64.
#ifndef M2T_MOMENT_TILE_H
#define M2T_MOMENT_TILE_H
#include <hip/hip_runtime.h>

namespace moment_tile {

// the sum of v over the N threads of a workgroup, to every thread: the wave by shuffles, the waves through red[N / 64] in index order
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

template <int WIN_, int TS_, int NT_, typename Raw_>
struct Tile {
  using Raw = Raw_;
  static constexpr int WIN = WIN_;              // taps of the window
  static constexpr int TS = TS_;                // output tile edge (pixels)
  static constexpr int NT = NT_;                // threads per workgroup
  static constexpr int TM = TS + WIN - 1;       // map entries per tile edge whose windows touch the tile
  static constexpr int TI = TM + WIN - 1;       // input samples per tile edge
  static constexpr size_t OFF_V = 0;                                             // 5 vertical passes; later (aliased) 3 transposed ones
  static constexpr size_t OFF_D = OFF_V + sizeof(double) * 5 * TM * TI;          // the three coefficient maps
  static constexpr size_t OFF_RED = OFF_D + sizeof(double) * 3 * TM * TM;
  static constexpr size_t OFF_X = OFF_RED + sizeof(double) * (NT / 64 > 8 ? NT / 64 : 8);
  static constexpr size_t OFF_Y = OFF_X + sizeof(Raw) * TI * TI;
  static constexpr size_t SMEM = OFF_Y + sizeof(Raw) * TI * TI;
  static_assert(SMEM <= 160 * 1024, "the tile does not fit the LDS of a CU");
  static_assert(3 * TS * TM <= 5 * TM * TI, "the transposed vertical pass is aliased on V");

  // (y0, x0): the tile's first pixel of the [H][W] plane; win.g[0 .. WIN) the taps.  SUM: sum[] = the workgroup's sums, to every
  // thread (SUM = false leaves sum[] alone).  Either way D is complete and V free for every thread on return.
  template <bool SUM, int NSUM, typename Taps, typename Load, typename Use, typename Map>
  static __device__ __forceinline__ void maps(unsigned char* smem, int H, int W, int y0, int x0, const Taps& win, Load load, Use use,
                                              Map map, double (&sum)[NSUM]) {
    double* const V = (double*)(smem + OFF_V);
    double* const D = (double*)(smem + OFF_D);
    double* const red = (double*)(smem + OFF_RED);
    Raw* const XR = (Raw*)(smem + OFF_X);
    Raw* const YR = (Raw*)(smem + OFF_Y);
    const int tid = threadIdx.x;
    const int Hm = H - WIN + 1, Wm = W - WIN + 1;
    const int my0 = y0 - (WIN - 1), mx0 = x0 - (WIN - 1);      // plane / map coordinates of local index 0 (may be negative)

    // 1. the input tiles, raw; 0 outside the plane
    for (int i = tid; i < TI * TI; i += NT) {
      const int r = i / TI, cc = i - r * TI;
      const int gy = my0 + r, gxx = mx0 + cc;
      const bool in = (gy >= 0) & (gy < H) & (gxx >= 0) & (gxx < W);       // (one flat predicate: one branch around the loads)
      Raw a = (Raw)0, b = (Raw)0;
      if (in) load(gy, gxx, a, b);
      XR[i] = a; YR[i] = b;
    }
    __syncthreads();

    // 2. vertical pass of u, v, uu, vv, uv
    for (int i = tid; i < TM * TI; i += NT) {
      const int r = i / TI, cc = i - r * TI;
      double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
#pragma unroll
      for (int t = 0; t < WIN; ++t) {
        const double g = win.g[t], u = use(XR[(r + t) * TI + cc]), v = (double)YR[(r + t) * TI + cc];
        a0 = fma(g, u, a0); a1 = fma(g, v, a1); a2 = fma(g, u * u, a2); a3 = fma(g, v * v, a3); a4 = fma(g, u * v, a4);
      }
      V[0 * TM * TI + i] = a0; V[1 * TM * TI + i] = a1; V[2 * TM * TI + i] = a2; V[3 * TM * TI + i] = a3; V[4 * TM * TI + i] = a4;
    }
    __syncthreads();

    // 3. horizontal pass, the point-wise map and its three coefficient maps
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
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
      double d[3];
      map(m, valid, valid && r >= WIN - 1 && cc >= WIN - 1, d, acc);
      D[0 * TM * TM + i] = d[0];
      D[1 * TM * TM + i] = d[1];
      D[2 * TM * TM + i] = d[2];
    }
    if (SUM) {                                                         // (the barriers of block_sum also close D and free V)
#pragma unroll
      for (int k = 0; k < NSUM; ++k) sum[k] = block_sum<NT>(acc[k], red);
    } else {
      __syncthreads();
    }
  }

  // After maps(): epi(gy, gxx, a0, a1, a2, x_raw, y_raw) for every pixel (gy, gxx) of the tile inside the plane that pass(x_raw)
  // lets through, a_k the transposed filter of coefficient map k there, x_raw / y_raw the samples load() gave.
  template <typename Taps, typename Pass, typename Epi>
  static __device__ __forceinline__ void grad(unsigned char* smem, int H, int W, int y0, int x0, const Taps& win, Pass pass, Epi epi) {
    double* const T = (double*)(smem + OFF_V);
    const double* const D = (const double*)(smem + OFF_D);
    const Raw* const XR = (const Raw*)(smem + OFF_X);
    const Raw* const YR = (const Raw*)(smem + OFF_Y);
    const int tid = threadIdx.x;

    // 4. transposed filter, vertical: pixel row y0 + r collects the map rows y0 + r - t (local r + WIN - 1 - t)
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

    // 5. transposed filter, horizontal; the epilogue of this tile's pixels
    for (int i = tid; i < TS * TS; i += NT) {
      const int r = i / TS, cc = i - r * TS;
      const int gy = y0 + r, gxx = x0 + cc;
      if (gy >= H || gxx >= W) continue;
      const int p = (r + WIN - 1) * TI + cc + WIN - 1;
      const Raw xr = XR[p];
      if (!pass(xr)) continue;
      double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
      for (int t = 0; t < WIN; ++t) {
        const double g = win.g[t];
        const int j = r * TM + cc + WIN - 1 - t;
        a0 = fma(g, T[j], a0); a1 = fma(g, T[TS * TM + j], a1); a2 = fma(g, T[2 * TS * TM + j], a2);
      }
      epi(gy, gxx, a0, a1, a2, xr, YR[p]);
    }
  }
};

}  // namespace moment_tile
#endif
