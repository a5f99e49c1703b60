// k_vif_loss.hip -- the information-fidelity loss term 1 - VIF (pixel domain, Sheikh & Bovik; piq.vif_p) with its gradient
// (include/m2t_vif.h has the definition; the reference imports VIFLoss from piq next to the pixel criteria, losses.py:8).
//
//   per image: u_0 = 255 / R * luminance(clamp(x)), v_0 likewise of y (never clamped);  u_s = (G_s * u_{s-1})[::2, ::2], windows of
//   17, 9, 5, 3 taps;  on every scale the moments a, b, c under G_s, the five-branch map t and the reference information d;
//   VIF_b = (sum t + EPS) / (sum d + EPS);  value = scale * sum_b (1 - VIF_b);  the denominator depends on y only.
//
// The gradient of scale s needs sum d of ALL scales: two phases, coupled through a per-image record in device memory.
//   pyramid   3 launches: level s from level s - 1, u and v together (m2t_vif_tile.h: pyr_tile, the decimated rows / columns only);
//             level 1 reads the fp32 images through clamp and luminance, levels 1 .. 3 are fp64 in scratch.
//   phase 1   one launch per scale, one workgroup per 16 x 16 tile: the five filtered moments in LDS, the tile's sums of t and d.
//   record    one workgroup per image folds the partial sums, scale 0 first, tiles in index order: sum t, sum d, VIF_b,
//             scale / (sum d + EPS); then one workgroup folds 1 - VIF_b into the loss.
//   phase 2   one launch per scale, 3 down to 0: the tile recomputes the moments, forms the three coefficient maps, filters them back
//             and adds the adjoint of (filter, decimate) of the parent level's gradient, gathered from scratch; scales 3 .. 1 store
//             fp64, scale 0 applies -scale / (sum d + EPS), the luminance weight, 255 / R and the clamp mask per channel and adds
//             into the destination with ONE fp32 rounding.
// Each output element of each level is written by exactly one thread, no atomics, fixed-order sums: two runs are bit-identical.
#include "m2t_common.h"
#include "m2t_kernels.h"
#include "m2t_vif_tile.h"
#include "../../include/m2t_vif.h"
#include <math.h>

namespace {

using namespace vif_tile;
template <int N> using TileN = Tile<N, 16, 256>;
constexpr int TS = 16;
static_assert(TileN<17>::SMEM <= 160 * 1024 && 2 * TileN<9>::SMEM <= 160 * 1024 && 4 * TileN<5>::SMEM <= 160 * 1024, "workgroups per CU");

constexpr int REC_T = 0, REC_D = 1, REC_VIF = 2, REC_COEF = 3, REC = 4;      // the record of one image, in doubles

using VifLayout = LevelledLayout;       // a = the u pyramid, b = the v pyramid, g = the gradient of a level

bool vif_layout(int B, int C, int H, int W, VifLayout& L) {
  if (B < 1 || B > 65535 || (C != 1 && C != 3) || H < MIN_SIDE || W < MIN_SIDE) return false;
  L.levels = SCALES;
  for (int s = 0; s < SCALES; ++s) {
    L.h[s] = s ? decimated_side(L.h[s - 1], win_len(s)) : H;
    L.w[s] = s ? decimated_side(L.w[s - 1], win_len(s)) : W;
    L.ty[s] = (L.h[s] + TS - 1) / TS;
    L.tx[s] = (L.w[s] + TS - 1) / TS;
  }
  levelled_layout_fill(L, (size_t)B, REC, 2);
  return true;
}

// the source of image b: src holds image 0, img_x / img_y / img_p are the image strides of x, y and the fp64 planes
template <bool L0>
__device__ __forceinline__ Src image_of(Src s, long long img_x, long long img_y, long long img_p, int b) {
  if (L0) { s.x += (long long)b * img_x; s.y += (long long)b * img_y; }
  else { s.u += (long long)b * img_p; s.v += (long long)b * img_p; }
  return s;
}

// One level of both pyramids: grid (ceil(Wo / 16), ceil(Ho / 16), B), 256 threads.
template <int N, bool L0>
__global__ __launch_bounds__(256) void vif_pyramid_kernel(Src src, long long img_x, long long img_y, long long img_p, int Hi, int Wi,
                                                          int Ho, int Wo, Taps win, double* __restrict__ uo, double* __restrict__ vo) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.z;
  const Src s = image_of<L0>(src, img_x, img_y, img_p, b);
  pyr_tile<N, L0>(smem, s, Hi, Wi, Ho, Wo, win, uo + (long long)b * Ho * Wo, vo + (long long)b * Ho * Wo);
}

// Phase 1, one scale: grid (tiles_x, tiles_y, B); partial [B][tiles_y][tiles_x][2] = the tile's sums of t and d.
template <int N, bool L0>
__global__ __launch_bounds__(256) void vif_value_kernel(Src src, long long img_x, long long img_y, long long img_p, int H, int W,
                                                        double nn, Taps win, double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char smem[];
  const Src s = image_of<L0>(src, img_x, img_y, img_p, blockIdx.z);
  double st = 0.0, sd = 0.0;
  TileN<N>::template maps<L0, true>(smem, s, H, W, blockIdx.y * TS, blockIdx.x * TS, nn, win, st, sd);
  if (threadIdx.x == 0) {
    double* const p = partial + (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    p[0] = st; p[1] = sd;
  }
}

struct VifFold {             // partial sums of scale s: part[s] doubles into the scratch, nt[s] tiles per image
  long long part[SCALES];
  int nt[SCALES];
};

// One workgroup per image: sum t, sum d, VIF_b and the coefficient of phase 2.  Fixed order.
__global__ __launch_bounds__(256) void vif_record_kernel(double* __restrict__ scratch, VifFold f, long long rec_off, double scale,
                                                         double* __restrict__ per_image_out) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  double tt = 0.0, dd = 0.0;
#pragma unroll
  for (int s = 0; s < SCALES; ++s) {
    const double* const p = scratch + f.part[s] + (long long)b * f.nt[s] * 2;
    double a = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < f.nt[s]; i += 256) { a += p[2 * i]; c += p[2 * i + 1]; }
    tt += block_sum<256>(a, red);
    dd += block_sum<256>(c, red);
  }
  if (threadIdx.x != 0) return;
  double* const r = scratch + rec_off + (long long)b * REC;
  const double vif = (tt + EPS) / (dd + EPS);
  r[REC_T] = tt; r[REC_D] = dd; r[REC_VIF] = vif; r[REC_COEF] = scale / (dd + EPS);
  if (per_image_out) per_image_out[b] = vif;
}

// Phase 2, one scale: G_s(p) = d sum(t_s) / du_s(p) + sum over parents of g g G_{s+1} (gpar = NULL on the coarsest scale; NP = N_{s+1}).
// L0 = false: gout [B][H][W] = G_s.  L0 = true (scale 0): per channel, gx[p] += (float)(-coef_b * w_ch * k255 * G_0(p)) where the
// clamp passes, x's strides.
template <int N, int NP, bool L0>
__global__ __launch_bounds__(256) void vif_grad_kernel(Src src, long long img_x, long long img_y, long long img_p, int H, int W,
                                                       double nn, Taps win, Taps pwin, const double* __restrict__ rec,
                                                       const double* __restrict__ gpar, int Hp, int Wp, float* __restrict__ gx,
                                                       double* __restrict__ gout) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double pg[MAXWIN];
  const int b = blockIdx.z;
  if (threadIdx.x < MAXWIN) pg[threadIdx.x] = pwin.g[threadIdx.x];
  const Src s = image_of<L0>(src, img_x, img_y, img_p, b);
  const int y0 = blockIdx.y * TS, x0 = blockIdx.x * TS;
  double st, sd;
  TileN<N>::template maps<L0, false>(smem, s, H, W, y0, x0, nn, win, st, sd);
  const double* const gp = gpar ? gpar + (long long)b * Hp * Wp : nullptr;
  const double coef = L0 ? -rec[(long long)b * REC + REC_COEF] * s.k255 : 0.0;
  float* const gxp = L0 ? gx + (long long)b * img_x : nullptr;
  double* const gop = L0 ? nullptr : gout + (long long)b * H * W;
  TileN<N>::grad(smem, H, W, y0, x0, win, [=](int gy, int gxx, double d) {
    double g = d;
    if (gp) g += parent_gather<NP>(gp, Hp, Wp, pg, gy, gxx);
    if (L0) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (ch >= s.C) break;
        const long long o = (long long)ch * s.xs_ch + (long long)gy * s.xs_row + gxx;
        const float xv = s.x[o];
        if (s.clamp && !(xv >= 0.f && xv <= s.R)) continue;           // the clamp passes no gradient
        const double wch = s.C == 3 ? (ch == 0 ? 0.299 : ch == 1 ? 0.587 : 0.114) : 1.0;
        gxp[o] = gxp[o] + (float)(coef * wch * g);                    // one fp32 rounding, one fp32 add per element
      }
    } else {
      gop[(long long)gy * W + gxx] = g;
    }
  });
}

struct Run {                // what every launch of one call shares
  Src src0; long long img_x, img_y; int B; double nn; double* s; const VifLayout* L; hipStream_t st; Taps win[SCALES];
};

Src plane_src(const Run& r, int s) {
  Src p = r.src0;
  p.u = r.s + r.L->a[s]; p.v = r.s + r.L->b[s]; p.row = r.L->w[s];
  return p;
}

template <int S>
int launch_pyramid(const Run& r) {          // level S from level S - 1
  constexpr int N = win_len(S);
  const VifLayout& L = *r.L;
  auto k = vif_pyramid_kernel<N, S == 1>;
  if (int rc = ensure_lds(k, Pyr<N>::SMEM)) return rc;
  const dim3 grid((L.w[S] + PT - 1) / PT, (L.h[S] + PT - 1) / PT, r.B);
  k<<<grid, 256, Pyr<N>::SMEM, r.st>>>(S == 1 ? r.src0 : plane_src(r, S - 1), r.img_x, r.img_y, (long long)L.h[S - 1] * L.w[S - 1],
                                      L.h[S - 1], L.w[S - 1], L.h[S], L.w[S], r.win[S], r.s + L.a[S], r.s + L.b[S]);
  M2T_LAUNCH_CHECK();
  return 0;
}

template <int S>
int launch_value(const Run& r) {
  constexpr int N = win_len(S);
  const VifLayout& L = *r.L;
  auto k = vif_value_kernel<N, S == 0>;
  if (int rc = ensure_lds(k, TileN<N>::SMEM)) return rc;
  k<<<dim3(L.tx[S], L.ty[S], r.B), 256, TileN<N>::SMEM, r.st>>>(S == 0 ? r.src0 : plane_src(r, S), r.img_x, r.img_y,
                                                                 (long long)L.h[S] * L.w[S], L.h[S], L.w[S], r.nn, r.win[S],
                                                                 r.s + L.part[S]);
  M2T_LAUNCH_CHECK();
  return 0;
}

template <int S>
int launch_grad(const Run& r, float* gx) {
  constexpr int N = win_len(S), NP = S < SCALES - 1 ? win_len(S + 1) : 1;
  const VifLayout& L = *r.L;
  auto k = vif_grad_kernel<N, NP, S == 0>;
  if (int rc = ensure_lds(k, TileN<N>::SMEM)) return rc;
  const bool top = S == SCALES - 1;
  k<<<dim3(L.tx[S], L.ty[S], r.B), 256, TileN<N>::SMEM, r.st>>>(S == 0 ? r.src0 : plane_src(r, S), r.img_x, r.img_y,
                                                                 (long long)L.h[S] * L.w[S], L.h[S], L.w[S], r.nn, r.win[S],
                                                                 r.win[top ? S : S + 1], r.s + L.rec, top ? nullptr : r.s + L.g[S + 1],
                                                                 top ? 0 : L.h[S + 1], top ? 0 : L.w[S + 1], gx,
                                                                 S == 0 ? nullptr : r.s + L.g[S]);
  M2T_LAUNCH_CHECK();
  return 0;
}

}  // namespace

size_t vif_loss_scratch_bytes(int B, int C, int H, int W) {
  VifLayout L;
  return vif_layout(B, C, H, W, L) ? sizeof(double) * L.total : 0;
}

bool vif_loss_size_supported(int H, int W) { return H >= MIN_SIDE && W >= MIN_SIDE; }

// the one device routine behind m2t_vif_loss_tensor and m2t_vif_loss (arguments checked by the callers)
int launch_vif_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, double sigma_n_sq,
                    int clamp, double scale, float* gx_add, float* loss_out, double* per_image_out, int accumulate, void* scratch,
                    hipStream_t st) {
  VifLayout L;
  if (!vif_layout(B, C, H, W, L)) return m2t_set_error(M2T_ERR_ARG, "m2t_vif_loss: unsupported shape");
  Run r;
  r.src0 = Src{x, y, xs_img / C, xs_row, (long long)H * W, W, C, R, clamp, 255.0 / (double)R, nullptr, nullptr, 0};
  r.img_x = xs_img; r.img_y = (long long)C * H * W; r.B = B; r.nn = sigma_n_sq; r.s = (double*)scratch; r.L = &L; r.st = st;
  for (int s = 0; s < SCALES; ++s) {
    for (int k = 0; k < MAXWIN; ++k) r.win[s].g[k] = 0.0;
    make_taps(win_len(s), r.win[s].g);
  }
  if (int rc = launch_pyramid<1>(r)) return rc;
  if (int rc = launch_pyramid<2>(r)) return rc;
  if (int rc = launch_pyramid<3>(r)) return rc;
  if (int rc = launch_value<0>(r)) return rc;
  if (int rc = launch_value<1>(r)) return rc;
  if (int rc = launch_value<2>(r)) return rc;
  if (int rc = launch_value<3>(r)) return rc;
  VifFold f;
  for (int s = 0; s < SCALES; ++s) { f.part[s] = (long long)L.part[s]; f.nt[s] = L.ty[s] * L.tx[s]; }
  vif_record_kernel<<<B, 256, 0, st>>>(r.s, f, (long long)L.rec, scale, per_image_out);
  M2T_LAUNCH_CHECK();
  if (int rc = launch_loss_finish(r.s + L.rec + REC_VIF, B, REC, 1, scale, accumulate, loss_out, st)) return rc;      // sum_b (1 - VIF_b)
  if (!gx_add) return 0;
  if (int rc = launch_grad<3>(r, gx_add)) return rc;
  if (int rc = launch_grad<2>(r, gx_add)) return rc;
  if (int rc = launch_grad<1>(r, gx_add)) return rc;
  return launch_grad<0>(r, gx_add);
}

extern "C" size_t m2t_vif_loss_scratch_bytes(int B, int C, int H, int W) { return vif_loss_scratch_bytes(B, C, H, W); }

extern "C" size_t m2t_vif_loss_scratch_offset(int B, int C, int H, int W, int region, int level) {
  VifLayout L;
  return vif_layout(B, C, H, W, L) ? levelled_layout_offset(L, region, level) : (size_t)-1;
}

extern "C" int m2t_vif_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                                   float data_range, double sigma_n_sq, int clamp, double scale, float* gx_add, float* loss_out,
                                   double* per_image_out, int accumulate, void* scratch, void* stream) {
  const char* const shape = (B < 1 || B > 65535) ? "need 1 <= B <= 65535" :
                            (C != 1 && C != 3) ? "C must be 1 or 3 (luminance of a grey or an RGB image)" :
                            !vif_loss_size_supported(H, W) ? "H and W must be at least 41 (four scales under the 17 / 9 / 5 / 3-tap windows)" : nullptr;
  const char* const more = (!(sigma_n_sq > 0.0) || !isfinite(sigma_n_sq)) ? "sigma_n_sq must be a finite number > 0" : nullptr;
  if (int rc = loss_tensor_check(__func__, x, y, loss_out, scratch, C, H, W, x_image_stride, x_row_stride, data_range, shape, more))
    return rc;
  return launch_vif_loss(x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, sigma_n_sq, clamp ? 1 : 0, scale, gx_add, loss_out,
                         per_image_out, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}
