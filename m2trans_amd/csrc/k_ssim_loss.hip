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
#include "m2t_ssim_tile.h"
#include "../../include/m2t.h"
#include <math.h>

namespace {

using ssim_tile::block_sum;
using ssim_tile::WIN;
using SsimTaps = ssim_tile::Taps;
using SsimTile = ssim_tile::Tile<float, 32, 512>;      // (m2t_ssim_tile.h, shared with k_msssim_loss.hip, on m2t_moment_tile.h)
constexpr int TS = SsimTile::TS;       // output tile edge (pixels)
constexpr int NT = SsimTile::NT;       // threads per workgroup
// LDS: 151 392 B of the CU's 160 KB: one workgroup of 8 waves per CU.
constexpr size_t SSIM_SMEM = SsimTile::SMEM;
static_assert(SSIM_SMEM == 151392, "the LDS layout of the SSIM tile changed");

// grid (tiles_x, tiles_y, B * C).  x: [B][C][H][W] with strides (xs_img, xs_ch, xs_row, 1); y contiguous; gx (or NULL): x's strides.
// gcoef = -scale / R: gx[q] += (float)(gcoef * d sum(S) / dx_normalised(q)) where the clamp passes (or everywhere with clamp = 0).
__global__ __launch_bounds__(NT) void ssim_loss_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, int C, int H, int W,
                                                            long long xs_img, long long xs_ch, int xs_row, float R, int clamp,
                                                            double gcoef, SsimTaps win, float* __restrict__ gx,
                                                            double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int bc = blockIdx.z, b = bc / C, c = bc - b * C;
  const int y0 = blockIdx.y * TS, x0 = blockIdx.x * TS;
  const long long xoff = (long long)b * xs_img + (long long)c * xs_ch;
  // steps 1 - 3: the map, its coefficient maps, the sum of 1 - S over the map entries this tile owns
  const double tsum = SsimTile::maps<ssim_tile::MAP_SSIM_LOSS, true>(smem, x + xoff, xs_row, y + (long long)bc * H * W, W, H, W, y0, x0,
                                                                      R, clamp, win);
  if (threadIdx.x == 0) partial[((long long)bc * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tsum;
  if (!gx) return;
  // steps 4 - 5: the transposed filter; one fp32 rounding, one fp32 add per element
  float* const gp = gx + xoff;
  SsimTile::grad(smem, H, W, y0, x0, R, clamp, win, [=](int gy, int gxx, double d, float) {
    const long long o = (long long)gy * xs_row + gxx;
    gp[o] = gp[o] + (float)(gcoef * d);
  });
}

// loss = (accumulate ? loss : 0) + (float)(scale * sum_i v_i), v_i = p[i * stride] or 1 - p[i * stride]: one workgroup, fixed order
__global__ __launch_bounds__(256) void loss_term_finish_kernel(const double* __restrict__ p, long long n, long long stride, int one_minus,
                                                          double scale, int accumulate, float* __restrict__ loss) {
  __shared__ double red[4];
  double a = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) a += one_minus ? 1.0 - p[i * stride] : p[i * stride];
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

// the dependency's window, exp(-(i-5)^2 / (2 sigma^2)) normalised, as torch builds it in fp32 (torch.exp, torch.sum) -- the bits of
// pytorch_msssim's own taps.  The built-in taps of m2t_eval_metrics (libm exp, sequential fp32 sum) differ from these in the last bit
// of five of them (1e-7): that moves the window's sum and with it s = E[x^2] - mu^2 by 1e-6 of the C2-sized variances.
void ssim_loss_taps(double* g11) {
  static const float kTaps[WIN / 2 + 1] = {0.0010283803567290306f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f, 0.21300552785396576f, 0.26601171493530273f};
  for (int i = 0; i < WIN; ++i) g11[i] = (double)kTaps[i <= WIN / 2 ? i : WIN - 1 - i];
}

// the one device routine behind m2t_ssim_loss_tensor and m2t_ssim_loss (arguments checked by the callers)
int launch_ssim_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                     double scale, float* gx_add, float* loss_out, int accumulate, void* scratch, hipStream_t st) {
  SsimTaps win;
  ssim_loss_taps(win.g);
  const int tx = (W + TS - 1) / TS, ty = (H + TS - 1) / TS;
  if (int rc = m2t_ensure_dynamic_lds((const void*)ssim_loss_tile_kernel, (int)SSIM_SMEM)) return rc;
  ssim_loss_tile_kernel<<<dim3(tx, ty, B * C), NT, SSIM_SMEM, st>>>(x, y, C, H, W, xs_img, xs_img / C, xs_row, R, clamp,
                                                                     -scale / (double)R, win, gx_add, (double*)scratch);
  M2T_LAUNCH_CHECK();
  return launch_loss_finish((const double*)scratch, (long long)B * C * tx * ty, 1, 0, scale, accumulate, loss_out, st);
}

int launch_loss_finish(const double* p, long long n, long long stride, int one_minus, double scale, int accumulate, float* loss_out,
                       hipStream_t st) {
  loss_term_finish_kernel<<<1, 256, 0, st>>>(p, n, stride, one_minus, scale, accumulate, loss_out);
  M2T_LAUNCH_CHECK();
  return 0;
}

void levelled_layout_fill(LevelledLayout& L, size_t items, int rec, int sums) {
  size_t off = 0;
  L.rec = off; off += items * rec;
  for (int l = 0; l < L.levels; ++l) { L.part[l] = off; off += items * L.ty[l] * L.tx[l] * sums; }
  for (size_t* plane : {L.a, L.b, L.g}) {
    plane[0] = 0;
    for (int l = 1; l < L.levels; ++l) { plane[l] = off; off += items * L.h[l] * L.w[l]; }
  }
  L.total = off;
}

size_t levelled_layout_offset(const LevelledLayout& L, int region, int level) {
  if (level < 0 || level >= L.levels) return (size_t)-1;
  if (region == 0) return sizeof(double) * L.rec;
  if (region == 1) return sizeof(double) * L.part[level];
  if (level < 1) return (size_t)-1;
  if (region == 2) return sizeof(double) * L.a[level];
  if (region == 3) return sizeof(double) * L.b[level];
  if (region == 4) return sizeof(double) * L.g[level];
  return (size_t)-1;
}

int loss_tensor_check(const char* who, const float* x, const float* y, const float* loss_out, const void* scratch, int C, int H, int W,
                      long long x_image_stride, int x_row_stride, float data_range, const char* shape_refusal, const char* more_refusal) {
  if (!x || !y || !loss_out || !scratch) return m2t_set_error_at(M2T_ERR_ARG, who, "null argument");
  if (shape_refusal) return m2t_set_error_at(M2T_ERR_ARG, who, shape_refusal);       // (from here on C >= 1)
  if (!(data_range > 0.f) || !isfinite(data_range)) return m2t_set_error_at(M2T_ERR_ARG, who, "data_range must be a finite number > 0");
  if (more_refusal) return m2t_set_error_at(M2T_ERR_ARG, who, more_refusal);
  if (x_row_stride < W || x_image_stride % C != 0 || x_image_stride / C < (long long)(H - 1) * x_row_stride + W)
    return m2t_set_error_at(M2T_ERR_ARG, who, "strides of x do not hold a [C][H][W] image (channel stride = x_image_stride / C)");
  return 0;
}

extern "C" size_t m2t_ssim_loss_scratch_bytes(int B, int C, int H, int W) { return ssim_loss_scratch_bytes(B, C, H, W); }

extern "C" int m2t_ssim_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                                    float data_range, int clamp, double scale, float* gx_add, float* loss_out, int accumulate,
                                    void* scratch, void* stream) {
  const char* const shape = (B < 1 || C < 1 || (long long)B * C > 65535) ? "need 1 <= B * C <= 65535" :
                            (H < WIN || W < WIN) ? "H and W must be at least 11 (the window)" : nullptr;
  if (int rc = loss_tensor_check(__func__, x, y, loss_out, scratch, C, H, W, x_image_stride, x_row_stride, data_range, shape))
    return rc;
  return launch_ssim_loss(x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, scale, gx_add, loss_out,
                          accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}
