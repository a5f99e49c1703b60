// k_msssim_loss.hip -- the multi-scale structural loss term 1 - MS-SSIM with its gradient (include/m2t_msssim.h; reference
// losses.py:8 imports MultiScaleSSIMLoss from piq next to the pixel criteria).
//
//   per image and channel: x_0 = clamp(pre, 0, R) / R, y_0 = hr / R;  x_{l+1} = the 2 x 2 average of x_l (padding side % 2, zeros
//   counted), y likewise;  v_l = mean(A2 / B2) on level l < 4, v_4 = mean(A1 A2 / (B1 B2));  M = prod_l max(v_l, 0)^{w_l};
//   value = scale * sum_bc (1 - M_bc);   dM / dx_l = (w_l M / (v_l n_l)) d sum(map_l) / dx_l, carried down by the pooling's adjoint.
//
// The gradient of level l needs M, i.e. every level's mean: two phases, coupled through a per-(b,c) record in device memory.
//   pyramid   4 launches: level l+1 from level l, x and y together.  The levels are fp64 and UN-normalised (pooled clamp(pre), pooled
//             hr): sums of at most 4^l fp32 numbers times 4^-l, exact, and summed in the order of the restatement -- bit for bit.
//   phase 1   one launch per level: the tile of m2t_ssim_tile.h (level 0: the fp32 tile of the SSIM term, 32 x 32; levels 1 .. 4:
//             fp64 inputs staged in LDS, 16 x 16 tile, 74 464 B, two workgroups per CU) reduces the map to one partial sum per tile.
//   finalize  one workgroup per (b,c) folds the partial sums of the five levels in a fixed order and writes the record: the
//             coefficients c_l = w_l M / (v_l n_l), M, the alive flag, v_l; then one workgroup folds 1 - M_bc into the loss.
//   phase 2   one launch per level, coarsest first: the tile recomputes the coefficient maps, filters them back, scales by c_l read
//             from the record and adds a quarter of the parent element of level l+1; levels 4 .. 1 store fp64, level 0 adds into
//             the destination through the clamp mask with ONE fp32 rounding.  A (b,c) that the zero rule silences returns at once.
// Each output element of each level is written by exactly one thread, no atomics: two runs are bit-identical.
//
// Cost (derived): the filtering runs twice over 1.33x the pixels, about 2.7x the kernel time of the SSIM term; the alternative
// (keep the three unscaled filtered maps of phase 1 and only combine them in phase 2) would cost 3 x 8 B x 1.33 per pixel of scratch
// (400 MB at B = 16, 512 x 512) and was not taken.  Measured at that size: 1.84 ms for the 16 launches, 2.49x the SSIM term.
#include "m2t_common.h"
#include "m2t_kernels.h"
#include "m2t_ssim_tile.h"
#include "../../include/m2t_msssim.h"
#include <math.h>

namespace {

using ssim_tile::block_sum;
using ssim_tile::MAP_CS;
using ssim_tile::MAP_SSIM;
using ssim_tile::Taps;
using ssim_tile::WIN;
using Tile0 = ssim_tile::Tile<float, 32, 512>;      // level 0: the tile of the SSIM term
using TileP = ssim_tile::Tile<double, 16, 256>;     // levels 1 .. 4: fp64 inputs
static_assert(TileP::SMEM <= 80 * 1024, "two workgroups of the fp64 tile per CU");

constexpr int LEVELS = 5;
constexpr int MIN_SIDE = (WIN - 1) * 16 + 1;        // 161: level 4 still holds one window
// the record of one (b,c), in doubles
constexpr int REC_COEF = 0, REC_M = 5, REC_ALIVE = 6, REC_V = 7, REC = 12;

using MsLayout = LevelledLayout;        // a = the x pyramid, b = the y pyramid, g = the gradient of a level

bool ms_layout(int B, int C, int H, int W, MsLayout& L) {
  if (B < 1 || C < 1 || (long long)B * C > 65535 || H < MIN_SIDE || W < MIN_SIDE) return false;
  L.levels = LEVELS;
  for (int l = 0; l < LEVELS; ++l) {
    L.h[l] = l ? L.h[l - 1] / 2 + L.h[l - 1] % 2 : H;
    L.w[l] = l ? L.w[l - 1] / 2 + L.w[l - 1] % 2 : W;
    const int ts = l ? TileP::TS : Tile0::TS;
    L.ty[l] = (L.h[l] + ts - 1) / ts;
    L.tx[l] = (L.w[l] + ts - 1) / ts;
  }
  levelled_layout_fill(L, (size_t)B * C, REC, 1);
  return true;
}

// One level of both pyramids: grid (ceil(Wo / 32), ceil(Ho / 8), B * C), block (32, 8).  x [B][C][H][W] with strides (xs_img, xs_ch,
// xs_row, 1), clamped to [0, R] first when clamp; y contiguous.  Output (oy, ox) = ((a + b) + c) + d) / 4 over the cell whose first
// member is (2 oy - H % 2, 2 ox - W % 2), row-major, members outside the image counting as 0.
template <typename TIn>
__global__ __launch_bounds__(256) void msssim_pool_kernel(const TIn* __restrict__ x, const TIn* __restrict__ y, int C, int H, int W,
                                                          long long xs_img, long long xs_ch, int xs_row, TIn R, int clamp,
                                                          double* __restrict__ xo, double* __restrict__ yo, int Ho, int Wo) {
  const int ox = blockIdx.x * 32 + threadIdx.x, oy = blockIdx.y * 8 + threadIdx.y;
  if (ox >= Wo || oy >= Ho) return;
  const int bc = blockIdx.z, b = bc / C, c = bc - b * C;
  const TIn* const xp = x + (long long)b * xs_img + (long long)c * xs_ch;
  const TIn* const yp = y + (long long)bc * H * W;
  const int iy0 = 2 * oy - (H & 1), ix0 = 2 * ox - (W & 1);
  double u[4], v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int gy = iy0 + (k >> 1), gxx = ix0 + (k & 1);
    const bool in = gy >= 0 && gy < H && gxx >= 0 && gxx < W;
    TIn a = in ? xp[(long long)gy * xs_row + gxx] : (TIn)0;
    if (clamp) a = ssim_tile::clamp_to(a, R);
    u[k] = (double)a;
    v[k] = in ? (double)yp[(long long)gy * W + gxx] : 0.0;
  }
  const long long o = ((long long)bc * Ho + oy) * Wo + ox;
  xo[o] = (((u[0] + u[1]) + u[2]) + u[3]) * 0.25;
  yo[o] = (((v[0] + v[1]) + v[2]) + v[3]) * 0.25;
}

// Phase 1, one level: grid (tiles_x, tiles_y, B * C); partial [B*C][tiles_y][tiles_x] = the tile's sum of the map (cs or SSIM).
template <typename T, int KIND>
__global__ __launch_bounds__(T::NT) void msssim_value_kernel(const typename T::In* __restrict__ x,
                                                             const typename T::In* __restrict__ y, int C, int H, int W,
                                                             long long xs_img, long long xs_ch, int xs_row, typename T::In R,
                                                             int clamp, Taps win, double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int bc = blockIdx.z, b = bc / C, c = bc - b * C;
  const double tsum = T::template maps<KIND, true>(smem, x + (long long)b * xs_img + (long long)c * xs_ch, xs_row,
                                                   y + (long long)bc * H * W, W, H, W, blockIdx.y * T::TS, blockIdx.x * T::TS, R, clamp, win);
  if (threadIdx.x == 0) partial[((long long)bc * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tsum;
}

struct MsFinalize {          // partial sums of level l: part[l] doubles into the scratch, nt[l] per (b,c); n[l] map entries
  long long part[LEVELS];
  int nt[LEVELS];
  double n[LEVELS];
};

// One workgroup per (b,c): v_l, M, the coefficients of phase 2.  Fixed order.
__global__ __launch_bounds__(256) void msssim_record_kernel(double* __restrict__ scratch, MsFinalize f, long long rec_off,
                                                            double* __restrict__ per_channel_out) {
  __shared__ double red[4];
  const int bc = blockIdx.x;
  double v[LEVELS];
#pragma unroll
  for (int l = 0; l < LEVELS; ++l) {
    const double* const p = scratch + f.part[l] + (long long)bc * f.nt[l];
    double a = 0.0;
    for (int i = threadIdx.x; i < f.nt[l]; i += 256) a += p[i];
    v[l] = block_sum<256>(a, red) / f.n[l];
  }
  if (threadIdx.x != 0) return;
  const double w[LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  bool alive = true;
  double M = 1.0;
#pragma unroll
  for (int l = 0; l < LEVELS; ++l) {
    alive = alive && v[l] > 0.0;
    M *= pow(fmax(v[l], 0.0), w[l]);
  }
  if (!alive) M = 0.0;                       // (a NaN mean lands here too: no gradient, M = 0)
  double* const r = scratch + rec_off + (long long)bc * REC;
#pragma unroll
  for (int l = 0; l < LEVELS; ++l) {
    r[REC_COEF + l] = alive ? w[l] * M / (v[l] * f.n[l]) : 0.0;
    r[REC_V + l] = v[l];
  }
  r[REC_M] = M;
  r[REC_ALIVE] = alive ? 1.0 : 0.0;
  if (per_channel_out) per_channel_out[bc] = M;
}

// Phase 2, one level: G_l(q) = c_l * d sum(map_l) / dx_l(q) + G_{l+1}(parent of q) / 4  (gpar = NULL on the coarsest level).
// TOP = false: gout [B*C][H][W] = G_l.  TOP = true (level 0): gx[q] += (float)(gcoef * G_0(q)) where the clamp passes, x's strides.
template <typename T, int KIND, bool TOP>
__global__ __launch_bounds__(T::NT) void msssim_grad_kernel(const typename T::In* __restrict__ x,
                                                            const typename T::In* __restrict__ y, int C, int H, int W,
                                                            long long xs_img, long long xs_ch, int xs_row, typename T::In R,
                                                            int clamp, Taps win, const double* __restrict__ rec, int level,
                                                            const double* __restrict__ gpar, int Hp, int Wp, double gcoef,
                                                            float* __restrict__ gx, double* __restrict__ gout) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int bc = blockIdx.z, b = bc / C, c = bc - b * C;
  const double* const r = rec + (long long)bc * REC;
  if (r[REC_ALIVE] == 0.0) return;                 // the zero rule: nothing is added for this (image, channel)
  const double cl = r[REC_COEF + level];
  const int y0 = blockIdx.y * T::TS, x0 = blockIdx.x * T::TS;
  const long long xoff = (long long)b * xs_img + (long long)c * xs_ch;
  T::template maps<KIND, false>(smem, x + xoff, xs_row, y + (long long)bc * H * W, W, H, W, y0, x0, R, clamp, win);
  const double* const gp = gpar ? gpar + (long long)bc * Hp * Wp : nullptr;
  const int py = H & 1, px = W & 1;                // the parent of (i, j) is ((i + H % 2) / 2, (j + W % 2) / 2)
  float* const gxp = TOP ? gx + xoff : nullptr;
  double* const gop = TOP ? nullptr : gout + (long long)bc * H * W;
  T::grad(smem, H, W, y0, x0, R, clamp, win, [=](int gy, int gxx, double d, typename T::In) {
    double g = cl * d;
    if (gp) g += 0.25 * gp[(long long)((gy + py) >> 1) * Wp + ((gxx + px) >> 1)];
    if (TOP) {
      const long long o = (long long)gy * xs_row + gxx;
      gxp[o] = gxp[o] + (float)(gcoef * g);          // one fp32 rounding, one fp32 add per element
    } else {
      gop[(long long)gy * W + gxx] = g;
    }
  });
}

}  // namespace

size_t msssim_loss_scratch_bytes(int B, int C, int H, int W) {
  MsLayout L;
  return ms_layout(B, C, H, W, L) ? sizeof(double) * L.total : 0;
}

bool msssim_loss_size_supported(int H, int W) { return H >= MIN_SIDE && W >= MIN_SIDE; }

// the one device routine behind m2t_msssim_loss_tensor and m2t_msssim_loss (arguments checked by the callers)
int launch_msssim_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                       double scale, float* gx_add, float* loss_out, double* per_channel_out, int accumulate, void* scratch,
                       hipStream_t st) {
  MsLayout L;
  if (!ms_layout(B, C, H, W, L)) return m2t_set_error(M2T_ERR_ARG, "m2t_msssim_loss: unsupported shape");
  Taps win;
  ssim_loss_taps(win.g);
  double* const s = (double*)scratch;
  const int planes = B * C;
  const double Rd = (double)R;
  auto v0 = msssim_value_kernel<Tile0, MAP_CS>;
  auto vp = msssim_value_kernel<TileP, MAP_CS>;
  auto v4 = msssim_value_kernel<TileP, MAP_SSIM>;
  if (int rc = ensure_lds(v0, Tile0::SMEM)) return rc;
  if (int rc = ensure_lds(vp, TileP::SMEM)) return rc;
  if (int rc = ensure_lds(v4, TileP::SMEM)) return rc;

  // the pyramids
  for (int l = 1; l < LEVELS; ++l) {
    const dim3 grid((L.w[l] + 31) / 32, (L.h[l] + 7) / 8, planes);
    if (l == 1)
      msssim_pool_kernel<float><<<grid, dim3(32, 8), 0, st>>>(x, y, C, H, W, xs_img, xs_img / C, xs_row, R, clamp, s + L.a[1], s + L.b[1],
                                                              L.h[1], L.w[1]);
    else
      msssim_pool_kernel<double><<<grid, dim3(32, 8), 0, st>>>(s + L.a[l - 1], s + L.b[l - 1], C, L.h[l - 1], L.w[l - 1],
                                                               (long long)C * L.h[l - 1] * L.w[l - 1], (long long)L.h[l - 1] * L.w[l - 1],
                                                               L.w[l - 1], Rd, 0, s + L.a[l], s + L.b[l], L.h[l], L.w[l]);
    M2T_LAUNCH_CHECK();
  }

  // phase 1: the five means
  MsFinalize f;
  for (int l = 0; l < LEVELS; ++l) {
    const dim3 grid(L.tx[l], L.ty[l], planes);
    const long long hw = (long long)L.h[l] * L.w[l];
    if (l == 0)
      v0<<<grid, Tile0::NT, Tile0::SMEM, st>>>(x, y, C, H, W, xs_img, xs_img / C, xs_row, R, clamp, win, s + L.part[0]);
    else
      (*(l < LEVELS - 1 ? vp : v4))<<<grid, TileP::NT, TileP::SMEM, st>>>(s + L.a[l], s + L.b[l], C, L.h[l], L.w[l], C * hw, hw, L.w[l],
                                                                         Rd, 0, win, s + L.part[l]);
    M2T_LAUNCH_CHECK();
    f.part[l] = (long long)L.part[l];
    f.nt[l] = L.ty[l] * L.tx[l];
    f.n[l] = (double)(L.h[l] - WIN + 1) * (double)(L.w[l] - WIN + 1);
  }
  msssim_record_kernel<<<planes, 256, 0, st>>>(s, f, (long long)L.rec, per_channel_out);
  M2T_LAUNCH_CHECK();
  if (int rc = launch_loss_finish(s + L.rec + REC_M, planes, REC, 1, scale, accumulate, loss_out, st)) return rc;      // sum_bc (1 - M_bc)
  if (!gx_add) return 0;

  // phase 2: the gradient, coarsest level first
  auto g4 = msssim_grad_kernel<TileP, MAP_SSIM, false>;
  auto gp = msssim_grad_kernel<TileP, MAP_CS, false>;
  auto g0 = msssim_grad_kernel<Tile0, MAP_CS, true>;
  if (int rc = ensure_lds(g4, TileP::SMEM)) return rc;
  if (int rc = ensure_lds(gp, TileP::SMEM)) return rc;
  if (int rc = ensure_lds(g0, Tile0::SMEM)) return rc;
  for (int l = LEVELS - 1; l >= 1; --l) {
    const dim3 grid(L.tx[l], L.ty[l], planes);
    const long long hw = (long long)L.h[l] * L.w[l];
    const bool top = l == LEVELS - 1;
    (*(top ? g4 : gp))<<<grid, TileP::NT, TileP::SMEM, st>>>(s + L.a[l], s + L.b[l], C, L.h[l], L.w[l], C * hw, hw, L.w[l], Rd, 0, win,
                                                         s + L.rec, l, top ? nullptr : s + L.g[l + 1], top ? 0 : L.h[l + 1],
                                                         top ? 0 : L.w[l + 1], 0.0, nullptr, s + L.g[l]);
    M2T_LAUNCH_CHECK();
  }
  g0<<<dim3(L.tx[0], L.ty[0], planes), Tile0::NT, Tile0::SMEM, st>>>(x, y, C, H, W, xs_img, xs_img / C, xs_row, R, clamp, win, s + L.rec, 0,
                                                                     s + L.g[1], L.h[1], L.w[1], -scale / (double)R, gx_add, nullptr);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t m2t_msssim_loss_scratch_bytes(int B, int C, int H, int W) { return msssim_loss_scratch_bytes(B, C, H, W); }

extern "C" size_t m2t_msssim_loss_scratch_offset(int B, int C, int H, int W, int region, int level) {
  MsLayout L;
  return ms_layout(B, C, H, W, L) ? levelled_layout_offset(L, region, level) : (size_t)-1;
}

extern "C" int m2t_msssim_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride,
                                      int x_row_stride, float data_range, int clamp, double scale, float* gx_add, float* loss_out,
                                      double* per_channel_out, int accumulate, void* scratch, void* stream) {
  const char* const shape = (B < 1 || C < 1 || (long long)B * C > 65535) ? "need 1 <= B * C <= 65535" :
                            !msssim_loss_size_supported(H, W) ? "H and W must be larger than 160 (five levels under the 11-tap window)" : nullptr;
  if (int rc = loss_tensor_check(__func__, x, y, loss_out, scratch, C, H, W, x_image_stride, x_row_stride, data_range, shape))
    return rc;
  return launch_msssim_loss(x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, scale, gx_add, loss_out,
                            per_channel_out, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}
