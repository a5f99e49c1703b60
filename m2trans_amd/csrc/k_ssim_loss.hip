// k_ssim_loss.hip -- the structural loss term 1 - SSIM with its gradient (reference losses.py:8 imports SSIMLoss / MultiScaleSSIMLoss
// from piq next to the pixel criteria; utils.py:232-234 scores every epoch by pytorch_msssim.ssim).
//
//   per channel, pytorch_msssim.ssim / piq.ssim(downsample=False) form:  x = clamp(pre, 0, R) / R,  y = hr / R  (data_range 1),
//   G = separable 11-tap Gaussian sigma 1.5 (the fp32 window as torch builds it, widened), VALID: map (H-10) x (W-10);
//   m1 = G*x, m2 = G*y, s1 = G*(x^2) - m1^2, s2 = G*(y^2) - m2^2, s12 = G*(xy) - m1 m2;  C1 = 1e-4, C2 = 9e-4;
//   A1 = 2 m1 m2 + C1, A2 = 2 s12 + C2, B1 = m1^2 + m2^2 + C1, B2 = s1 + s2 + C2;  S = A1 A2 / (B1 B2)  (no non-negativity clamp);
//   value = scale * sum_map (1 - S).
//   dE = -A1 A2 / (B1 B2^2), dF = 2 A1 / (B1 B2), dM = 2 m2 (A2 - A1) / (B1 B2) - 2 m1 S / B1 + 2 m1 S / B2;
//   d sum(S) / dx(q) = (G^T*dM)(q) + 2 x(q) (G^T*dE)(q) + y(q) (G^T*dF)(q),   G^T* = full correlation, zeros outside the map.
//
// piq.SSIMLoss's default downsample=True (an average pooling by max(1, round(min(H, W) / 256)) in front) is NOT part of this kernel.
//
// Everything between the fp32 inputs (widened: exact) and the one fp32 rounding of each gradient value is fp64, as in
// eval_ssim_y_kernel and for its reason: s = E[x^2] - mu^2 cancels, and late in training (SR close to HR) the variances are far
// below C2 -- an fp32 evaluation of this gradient is already off by 5e-6 of its largest entry on rough images.
//
// Shape: ONE kernel per 32 x 32 tile of the image plane.  It holds the 52 x 52 input tile of both images in LDS as fp32, recomputes
// the SSIM map and the three coefficient maps on the 42 x 42 map entries whose windows touch the tile (about 1.7x redundant
// filtering, no intermediate in HBM), filters them back and adds the gradient of its own 1024 pixels: each output element is
// written by exactly one thread.  A tile sums 1 - S over the map entries whose top-left pixel it owns; the partial sums go to a
// scratch array and are folded by one workgroup in a fixed order (as eval_finalize_kernel): deterministic, no atomics.
#include "m2t_common.h"
#include "m2t_kernels.h"
#include "../../include/m2t.h"
#include <math.h>

namespace {

constexpr int WIN = 11;
constexpr int TS = 32;                 // output tile edge (pixels)
constexpr int TM = TS + WIN - 1;       // 42: map entries per tile edge whose windows touch the tile
constexpr int TI = TM + WIN - 1;       // 52: input samples per tile edge
constexpr int NT = 512;                // threads per workgroup

// LDS (bytes): raw x | y tiles fp32; V = vertical pass of x, y, xx, yy, xy, later (aliased) the vertical pass of the transposed
// filter; D = dM | dE | dF.  151 376 of the CU's 160 KB: one workgroup of 8 waves per CU.
constexpr size_t OFF_V = 0;
constexpr size_t OFF_D = OFF_V + sizeof(double) * 5 * TM * TI;
constexpr size_t OFF_RED = OFF_D + sizeof(double) * 3 * TM * TM;
constexpr size_t OFF_X = OFF_RED + sizeof(double) * (NT / 64);
constexpr size_t OFF_Y = OFF_X + sizeof(float) * TI * TI;
constexpr size_t SSIM_SMEM = OFF_Y + sizeof(float) * TI * TI;
static_assert(SSIM_SMEM <= 160 * 1024, "the tile does not fit the LDS of a CU");
static_assert(3 * TS * TM <= 5 * TM * TI, "the transposed vertical pass is aliased on V");

struct SsimTaps { double g[WIN]; };

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

// grid (tiles_x, tiles_y, B * C).  x: [B][C][H][W] with strides (xs_img, xs_ch, xs_row, 1); y contiguous; gx (or NULL): x's strides.
// gcoef = -scale / R: gx[q] += (float)(gcoef * d sum(S) / dx_normalised(q)) where the clamp passes (or everywhere with clamp = 0).
__global__ __launch_bounds__(NT) void ssim_loss_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, int C, int H, int W,
                                                            long long xs_img, long long xs_ch, int xs_row, float R, int clamp,
                                                            double gcoef, SsimTaps win, float* __restrict__ gx,
                                                            double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* const V = (double*)(smem + OFF_V);
  double* const D = (double*)(smem + OFF_D);
  double* const red = (double*)(smem + OFF_RED);
  float* const XR = (float*)(smem + OFF_X);
  float* const YR = (float*)(smem + OFF_Y);
  const int tid = threadIdx.x;
  const int bc = blockIdx.z, b = bc / C, c = bc - b * C;
  const int Hm = H - WIN + 1, Wm = W - WIN + 1;
  const int y0 = blockIdx.y * TS, x0 = blockIdx.x * TS;
  const int my0 = y0 - (WIN - 1), mx0 = x0 - (WIN - 1);      // image / map coordinates of local index 0 (may be negative)
  const long long xoff = (long long)b * xs_img + (long long)c * xs_ch;
  const float* const xp = x + xoff;
  const float* const yp = y + (long long)bc * H * W;

  // 1. the input tiles, raw (the clamp is applied where a value is used: the mask of the gradient needs the raw one); 0 outside the image
  for (int i = tid; i < TI * TI; i += NT) {
    const int r = i / TI, cc = i - r * TI;
    const int gy = my0 + r, gxx = mx0 + cc;
    const bool in = gy >= 0 && gy < H && gxx >= 0 && gxx < W;
    XR[i] = in ? xp[(long long)gy * xs_row + gxx] : 0.f;
    YR[i] = in ? yp[(long long)gy * W + gxx] : 0.f;
  }
  __syncthreads();

  // 2. vertical pass of u, v, uu, vv, uv (u = clamp(pre), v = hr: unnormalised, the 1 / R factors are applied to the moments)
  for (int i = tid; i < TM * TI; i += NT) {
    const int r = i / TI, cc = i - r * TI;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
#pragma unroll
    for (int t = 0; t < WIN; ++t) {
      float uf = XR[(r + t) * TI + cc];
      if (clamp) uf = fminf(fmaxf(uf, 0.f), R);
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
    const double A1 = 2.0 * m1 * m2 + C1, A2 = 2.0 * s12 + C2, B1 = m1 * m1 + m2 * m2 + C1, B2 = s1 + s2 + C2;
    const double iB = 1.0 / (B1 * B2);
    const double S = A1 * A2 * iB;
    const double dM = 2.0 * m2 * (A2 - A1) * iB - 2.0 * m1 * S / B1 + 2.0 * m1 * S / B2;
    const double dE = -S / B2;
    const double dF = 2.0 * A1 * iB;
    D[0 * TM * TM + i] = valid ? dM : 0.0;
    D[1 * TM * TM + i] = valid ? dE : 0.0;
    D[2 * TM * TM + i] = valid ? dF : 0.0;
    if (valid && r >= WIN - 1 && cc >= WIN - 1) acc += 1.0 - S;      // the map entries this tile owns
  }
  const double tsum = block_sum<NT>(acc, red);                        // (its barriers also close D and free V)
  if (tid == 0) partial[((long long)bc * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tsum;
  if (!gx) return;

  // 4. transposed filter, vertical: pixel row y0 + r collects the map rows y0 + r - t (local r + 10 - t)
  double* const T = V;
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

  // 5. transposed filter, horizontal; the gradient of this tile's pixels: one fp32 rounding, one fp32 add per element
  float* const gp = gx + xoff;
  for (int i = tid; i < TS * TS; i += NT) {
    const int r = i / TS, cc = i - r * TS;
    const int gy = y0 + r, gxx = x0 + cc;
    if (gy >= H || gxx >= W) continue;
    const float uf = XR[(r + WIN - 1) * TI + cc + WIN - 1];
    if (clamp && !(uf >= 0.f && uf <= R)) continue;                   // the clamp passes no gradient (inclusive ends, as the pixel losses)
    double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
    for (int t = 0; t < WIN; ++t) {
      const double g = win.g[t];
      const int j = r * TM + cc + WIN - 1 - t;
      a0 = fma(g, T[j], a0); a1 = fma(g, T[TS * TM + j], a1); a2 = fma(g, T[2 * TS * TM + j], a2);
    }
    const double xn = (double)uf * iR, yn = (double)YR[(r + WIN - 1) * TI + cc + WIN - 1] * iR;
    const double d = a0 + 2.0 * xn * a1 + yn * a2;
    const long long o = (long long)gy * xs_row + gxx;
    gp[o] = gp[o] + (float)(gcoef * d);
  }
}

// loss = (accumulate ? loss : 0) + (float)(scale * sum(partial[0 .. n))): one workgroup, fixed order
__global__ __launch_bounds__(256) void ssim_loss_finish_kernel(const double* __restrict__ partial, long long n, double scale, int accumulate,
                                                               float* __restrict__ loss) {
  __shared__ double red[4];
  double a = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) a += partial[i];
  const double t = block_sum<256>(a, red);
  if (threadIdx.x == 0) {
    const float v = (float)(scale * t);
    loss[0] = accumulate ? loss[0] + v : v;
  }
}

}  // namespace

size_t ssim_loss_scratch_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || H < WIN || W < WIN) return 0;
  return sizeof(double) * (size_t)B * C * (size_t)((H + TS - 1) / TS) * (size_t)((W + TS - 1) / TS);
}

// the one device routine behind m2t_ssim_loss_tensor and m2t_ssim_loss (arguments checked by the callers)
int launch_ssim_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                     double scale, float* gx_add, float* loss_out, int accumulate, void* scratch, hipStream_t st) {
  // the dependency's window, exp(-(i-5)^2 / (2 sigma^2)) normalised, as torch builds it in fp32 (torch.exp, torch.sum) -- the bits of
  // pytorch_msssim's own taps.  The built-in taps of m2t_eval_metrics (libm exp, sequential fp32 sum) differ from these in the last bit
  // of five of them (1e-7): that moves the window's sum and with it s = E[x^2] - mu^2 by 1e-6 of the C2-sized variances.
  static const float kTaps[WIN / 2 + 1] = {0.0010283803567290306f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f, 0.21300552785396576f, 0.26601171493530273f};
  SsimTaps win;
  for (int i = 0; i < WIN; ++i) win.g[i] = (double)kTaps[i <= WIN / 2 ? i : WIN - 1 - i];
  const int tx = (W + TS - 1) / TS, ty = (H + TS - 1) / TS;
  if (int rc = m2t_ensure_dynamic_lds((const void*)ssim_loss_tile_kernel, (int)SSIM_SMEM)) return rc;
  ssim_loss_tile_kernel<<<dim3(tx, ty, B * C), NT, SSIM_SMEM, st>>>(x, y, C, H, W, xs_img, xs_img / C, xs_row, R, clamp,
                                                                     -scale / (double)R, win, gx_add, (double*)scratch);
  M2T_LAUNCH_CHECK();
  ssim_loss_finish_kernel<<<1, 256, 0, st>>>((const double*)scratch, (long long)B * C * tx * ty, scale, accumulate, loss_out);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t m2t_ssim_loss_scratch_bytes(int B, int C, int H, int W) { return ssim_loss_scratch_bytes(B, C, H, W); }

extern "C" int m2t_ssim_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                                    float data_range, int clamp, double scale, float* gx_add, float* loss_out, int accumulate,
                                    void* scratch, void* stream) {
  if (!x || !y || !loss_out || !scratch) return m2t_set_error(M2T_ERR_ARG, "m2t_ssim_loss_tensor: null argument");
  if (B < 1 || C < 1 || (long long)B * C > 65535) return m2t_set_error(M2T_ERR_ARG, "m2t_ssim_loss_tensor: need 1 <= B * C <= 65535");
  if (H < WIN || W < WIN) return m2t_set_error(M2T_ERR_ARG, "m2t_ssim_loss_tensor: H and W must be at least 11 (the window)");
  if (!(data_range > 0.f) || !isfinite(data_range)) return m2t_set_error(M2T_ERR_ARG, "m2t_ssim_loss_tensor: data_range must be a finite number > 0");
  if (x_row_stride < W || x_image_stride % C != 0 || x_image_stride / C < (long long)(H - 1) * x_row_stride + W)
    return m2t_set_error(M2T_ERR_ARG, "m2t_ssim_loss_tensor: strides of x do not hold a [C][H][W] image (channel stride = x_image_stride / C)");
  return launch_ssim_loss(x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, scale, gx_add, loss_out,
                          accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}
