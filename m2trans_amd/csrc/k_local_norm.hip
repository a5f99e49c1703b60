// k_local_norm.hip -- local-window InstanceNorm statistics and their apply (option "local_norm" of include/m2t.h: the Test-time Local
// Converter of Chu et al., ECCV 2022, for the InstanceNorm2d in front of every CFTM block).  Two launches per block, in front of the
// unchanged forward kernels; the per-thread text and the reasons for its shape are in m2t_local_norm_tile.h.
//   pass 1  horizontal sliding sums of x and x^2 -> hs (fp64 pairs)
//   pass 2  vertical sliding sums of hs, statistics, apply -> Xn (the plan's element type)
// Thread order: the 4-channel quarter of a 16-channel chunk fastest, then the column (pass 2) / the column segment (pass 1): in
// pass 2 a wave reads 4 KB of hs and 512 B (bf16) of X contiguously per row step; in pass 1 four lanes write 256 contiguous bytes.
#include "m2t_kernels.h"
#include "m2t_local_norm_tile.h"

using namespace ln_tile;

template <typename T>
__global__ void __launch_bounds__(256) local_norm_hsum_kernel(const T* __restrict__ X, double* __restrict__ hs, long long rows /* B * H */,
                                                              int W, int kw, int nseg) {
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int q = (int)(t & 3);
  t >>= 2;
  const int seg = (int)(t % nseg);
  t /= nseg;
  const long long row = t % rows;
  const long long chunk = t / rows;
  if (chunk >= 4) return;
  const size_t e = ((size_t)(chunk * rows + row) * W) * 16 + q * CPL;      // channel q * 4 of pixel (row, 0) of the chunk
  const int x0 = seg * SEGX;
  hsum_segment<T>(X + e, hs + 2 * e, x0, min(x0 + SEGX, W), W, kw);
}

template <typename T>
__global__ void __launch_bounds__(256) local_norm_vapply_kernel(const T* __restrict__ X, const double* __restrict__ hs, T* __restrict__ Xn,
                                                                int B, int H, int W, int kh, int nseg, double n) {
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int q = (int)(t & 3);
  t >>= 2;
  const int x = (int)(t % W);
  t /= W;
  const int seg = (int)(t % nseg);
  t /= nseg;
  const long long b = t % B;
  const long long chunk = t / B;
  if (chunk >= 4) return;
  const size_t e = (((size_t)(chunk * B + b) * H) * W + x) * 16 + q * CPL;   // channel q * 4 of pixel (0, x) of image b, chunk
  const int y0 = seg * SEGY;
  vapply_segment<T>(hs + 2 * e, X + e, Xn + e, y0, min(y0 + SEGY, H), H, W, kh, n);
}

int launch_local_norm(int dt, const void* X, void* hs, void* Xn, int B, int H, int W, int T, hipStream_t st) {
  if (!X || !hs || !Xn || B < 1 || H < 1 || W < 1 || T < 1) return m2t_set_error(-2, "local_norm: bad argument");
  const int kh = std::min(T, H), kw = std::min(T, W);
  const int nsx = ceil_div(W, SEGX), nsy = ceil_div(H, SEGY);
  const long long rows = (long long)B * H;
  const long long n1 = 4 * rows * nsx * 4, n2 = 4LL * B * nsy * W * 4;
  const long long g1 = ceil_divll(n1, 256), g2 = ceil_divll(n2, 256);
  if (g1 >= (1LL << 31) || g2 >= (1LL << 31)) return m2t_set_error(-2, "local_norm: map too large for one launch");
  const double n = (double)kh * (double)kw;
  if (dt == M2T_F32) {
    hipLaunchKernelGGL(local_norm_hsum_kernel<float>, dim3((unsigned)g1), dim3(256), 0, st, (const float*)X, (double*)hs, rows, W, kw, nsx);
    M2T_LAUNCH_CHECK();
    hipLaunchKernelGGL(local_norm_vapply_kernel<float>, dim3((unsigned)g2), dim3(256), 0, st, (const float*)X, (const double*)hs, (float*)Xn,
                       B, H, W, kh, nsy, n);
  } else {
    hipLaunchKernelGGL(local_norm_hsum_kernel<bf16_t>, dim3((unsigned)g1), dim3(256), 0, st, (const bf16_t*)X, (double*)hs, rows, W, kw, nsx);
    M2T_LAUNCH_CHECK();
    hipLaunchKernelGGL(local_norm_vapply_kernel<bf16_t>, dim3((unsigned)g2), dim3(256), 0, st, (const bf16_t*)X, (const double*)hs,
                       (bf16_t*)Xn, B, H, W, kh, nsy, n);
  }
  M2T_LAUNCH_CHECK();
  return 0;
}
