// k_consistency.hip -- LR-consistency (include/m2t_consistency.h has the definition): the loss term rho((D c(x) - y) / R) with its
// gradient through the adjoint of the bicubic down-sampler, D^T alone, and one iteration of back-projection.
//
//   forward   one workgroup per tile of 16 x 32 LR cells and plane (m2t_consistency_tile.h: down_tile): the clamped SR tile with its
//             mirrored halo in LDS, D in fp64, the residual; rho' (loss) or r (back-projection) to the fp64 plane in the scratch, the
//             tile's sums {sum rho, sum |r|, max |r|, sum r^2} to its slot.
//   fold      one workgroup folds the slots in tile order into loss_out / stats_out.
//   backward  (loss, only with a destination) one workgroup per tile of 32 x 64 SR pixels (adjoint_tile): D^T in gather form, the
//             clamp mask, one fp32 rounding, one read-add-write of the seed element.
//   update    (back-projection, only with update != 0) one workgroup per 16 x 16 LR cells (update_tile): U(r), the add, the clamp
//             and the store in one pass over SR.
// Each output element is written by exactly one thread, no atomics, fixed-order sums: two runs are bit-identical.
#include "m2t_common.h"
#include "m2t_kernels.h"
#include "m2t_consistency_tile.h"
#include "../../include/m2t_consistency.h"
#include <math.h>
#include <stdint.h>

namespace {

using namespace cons_tile;

struct ConsLayout { int ty, tx; long long planes; size_t plane, part, total; };      // offsets and total in doubles

bool cons_layout(int B, int C, int H, int W, int s, ConsLayout& L) {
  if (s < 2 || s > 4 || B < 1 || (C != 1 && C != 3) || (long long)B * C > 65535 || H < 1 || W < 1 || (long long)H * s > 16384 ||
      (long long)W * s > 16384)
    return false;
  L.planes = (long long)B * C;
  L.ty = ceil_div(H, Down<2>::TQH); L.tx = ceil_div(W, Down<2>::TQW);
  L.plane = 0;
  L.part = (size_t)L.planes * H * W;
  L.total = L.part + (size_t)L.planes * L.ty * L.tx * 4;
  return true;
}

// grid (tiles along W, tiles along H, B * C); x: plane z = (b, c) starts at b * xs_img + c * xs_ch
template <int S>
__global__ __launch_bounds__(256) void cons_down_kernel(const float* __restrict__ x, long long xs_img, long long xs_ch, int xs_row, int C,
                                                        const float* __restrict__ y, int H, int W, float R, int clamp, double iR,
                                                        double eps, int back_project, Taps taps, double* __restrict__ plane,
                                                        double* __restrict__ part) {
  __shared__ __align__(16) unsigned char smem[Down<S>::SMEM];
  const int z = blockIdx.z, b = z / C, c = z - b * C;
  double sums[4];
  down_tile<S>(smem, x + b * xs_img + c * xs_ch, xs_row, y + (long long)z * H * W, H, W, blockIdx.y * Down<S>::TQH,
               blockIdx.x * Down<S>::TQW, R, clamp, iR, eps, back_project, taps, plane + (long long)z * H * W, sums);
  if (threadIdx.x == 0) {
    double* const p = part + (((long long)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4;
    p[0] = sums[0]; p[1] = sums[1]; p[2] = sums[2]; p[3] = sums[3];
  }
}

__global__ __launch_bounds__(256) void cons_finish_kernel(const double* __restrict__ part, long long nt, double n, double scale,
                                                          int accumulate, float* __restrict__ loss_out, double* __restrict__ stats_out) {
  __shared__ double red[8];
  finish_tile(red, part, nt, n, scale, accumulate, loss_out, stats_out);
}

// grid (tiles along Ws, tiles along Hs, planes); xp (or nullptr) and op: plane z = (b, c) at b * img + c * ch, row stride `row`
template <int S, typename GT>
__global__ __launch_bounds__(256) void cons_adjoint_kernel(const GT* __restrict__ g, int H, int W, const float* __restrict__ x,
                                                           float* __restrict__ out, long long img, long long ch, int row, int C, float R,
                                                           int clamp, double coef, Taps taps, int accumulate) {
  __shared__ __align__(16) unsigned char smem[Adj<S>::SMEM];
  const int z = blockIdx.z, b = z / C, c = z - b * C;
  const long long off = b * img + c * ch;
  adjoint_tile<S, GT>(smem, g + (long long)z * H * W, H, W, blockIdx.y * Adj<S>::TH, blockIdx.x * Adj<S>::TW, x ? x + off : nullptr, row,
                      R, clamp, coef, taps, out + off, row, accumulate);
}

// grid (tiles along W, tiles along H, planes) of 16 x 16 LR cells
template <int S>
__global__ __launch_bounds__(256) void cons_update_kernel(const double* __restrict__ r, float* __restrict__ sr, int H, int W, float R,
                                                          double bR, int vec, Taps taps) {
  __shared__ __align__(16) unsigned char smem[Upd<S>::SMEM];
  const long long z = blockIdx.z;
  update_tile<S>(smem, r + z * H * W, sr + z * H * W * S * S, H, W, blockIdx.y * Up::TQ, blockIdx.x * Up::TQ, R, bR, vec, taps);
}

template <int S>
int launch_down(const float* x, long long xs_img, int xs_row, int C, const float* y, int H, int W, float R, int clamp, double eps,
                int back_project, const ConsLayout& L, double* sc, hipStream_t st) {
  const dim3 grid(L.tx, L.ty, (unsigned)L.planes);
  cons_down_kernel<S><<<grid, NT, 0, st>>>(x, xs_img, xs_img / C, xs_row, C, y, H, W, R, clamp, 1.0 / (double)R, eps, back_project,
                                           make_taps(S, false), sc + L.plane, sc + L.part);
  M2T_LAUNCH_CHECK();
  return 0;
}

template <int S, typename GT>
int launch_adjoint(const GT* g, int H, int W, long long planes, const float* x, float* out, long long img, int row, int C, float R,
                   int clamp, double coef, int accumulate, hipStream_t st) {
  const dim3 grid(ceil_div(W * S, Adj<S>::TW), ceil_div(H * S, Adj<S>::TH), (unsigned)planes);
  cons_adjoint_kernel<S, GT><<<grid, NT, 0, st>>>(g, H, W, x, out, img, img / C, row, C, R, clamp, coef, make_taps(S, false), accumulate);
  M2T_LAUNCH_CHECK();
  return 0;
}

template <int S>
int launch_update(const double* r, float* sr, int H, int W, long long planes, float R, double beta, hipStream_t st) {
  const dim3 grid(ceil_div(W, Up::TQ), ceil_div(H, Up::TQ), (unsigned)planes);
  const int vec = ((uintptr_t)sr & 15) == 0 && (W * S) % 4 == 0;
  cons_update_kernel<S><<<grid, NT, 0, st>>>(r, sr, H, W, R, beta * (double)R, vec, make_taps(S, true));
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_finish(const ConsLayout& L, int H, int W, double* sc, double scale, int accumulate, float* loss_out, double* stats_out,
                  hipStream_t st) {
  cons_finish_kernel<<<1, NT, 0, st>>>(sc + L.part, L.planes * L.ty * L.tx, (double)L.planes * H * W, scale, accumulate, loss_out,
                                       stats_out);
  M2T_LAUNCH_CHECK();
  return 0;
}

const char* cons_shape_refusal(int B, int C, int H, int W, int s) {
  return (s < 2 || s > 4) ? "scale_factor must be 2, 3 or 4" :
         (C != 1 && C != 3) ? "C must be 1 or 3" :
         (B < 1 || (long long)B * C > 65535) ? "need B >= 1 and B * C <= 65535" :
         (H < 1 || W < 1) ? "H and W must be at least 1" :
         ((long long)H * s > 16384 || (long long)W * s > 16384) ? "SR side above 16384" : nullptr;
}

}  // namespace

size_t consistency_scratch_bytes(int B, int C, int H, int W, int s) {
  ConsLayout L;
  return cons_layout(B, C, H, W, s, L) ? sizeof(double) * L.total : 0;
}

// the one device routine behind m2t_consistency_loss_tensor and m2t_consistency_loss (arguments checked by the callers)
int launch_consistency_loss(const float* x, const float* y, int B, int C, int H, int W, int s, long long xs_img, int xs_row, float R,
                            int clamp, double eps, double scale, float* gx_add, float* loss_out, double* stats_out, int accumulate,
                            void* scratch, hipStream_t st) {
  ConsLayout L;
  if (!cons_layout(B, C, H, W, s, L)) return m2t_set_error(M2T_ERR_ARG, "m2t_consistency_loss: unsupported shape");
  double* const sc = (double*)scratch;
  int rc = s == 2 ? launch_down<2>(x, xs_img, xs_row, C, y, H, W, R, clamp, eps, 0, L, sc, st) :
           s == 3 ? launch_down<3>(x, xs_img, xs_row, C, y, H, W, R, clamp, eps, 0, L, sc, st) :
                    launch_down<4>(x, xs_img, xs_row, C, y, H, W, R, clamp, eps, 0, L, sc, st);
  if (rc) return rc;
  if ((rc = launch_finish(L, H, W, sc, scale, accumulate, loss_out, stats_out, st))) return rc;
  if (!gx_add) return 0;
  const double coef = scale / (double)R;
  const double* const g = sc + L.plane;
  return s == 2 ? launch_adjoint<2, double>(g, H, W, L.planes, x, gx_add, xs_img, xs_row, C, R, clamp, coef, 1, st) :
         s == 3 ? launch_adjoint<3, double>(g, H, W, L.planes, x, gx_add, xs_img, xs_row, C, R, clamp, coef, 1, st) :
                  launch_adjoint<4, double>(g, H, W, L.planes, x, gx_add, xs_img, xs_row, C, R, clamp, coef, 1, st);
}

extern "C" size_t m2t_consistency_scratch_bytes(int B, int C, int H, int W, int scale) {
  return consistency_scratch_bytes(B, C, H, W, scale);
}

extern "C" int m2t_imresize_adjoint_f32(const float* g, int planes, int h, int w, float* out, int scale, int accumulate, void* stream) {
  const char* const bad = (!g || !out) ? "null pointer" :
                          (scale < 2 || scale > 4) ? "scale must be 2, 3 or 4" :
                          (planes < 1 || planes > 65535) ? "planes must be 1 .. 65535" :
                          (h < 1 || w < 1) ? "h and w must be at least 1" :
                          ((long long)h * scale > 16384 || (long long)w * scale > 16384) ? "output side above 16384" : nullptr;
  if (bad) return m2t_set_error_at(M2T_ERR_ARG, __func__, bad);
  hipStream_t st = (hipStream_t)stream;
  const long long img = (long long)h * scale * w * scale;
  const int row = w * scale, acc = accumulate ? 1 : 0;
  return scale == 2 ? launch_adjoint<2, float>(g, h, w, planes, nullptr, out, img, row, 1, 1.f, 0, 1.0, acc, st) :
         scale == 3 ? launch_adjoint<3, float>(g, h, w, planes, nullptr, out, img, row, 1, 1.f, 0, 1.0, acc, st) :
                      launch_adjoint<4, float>(g, h, w, planes, nullptr, out, img, row, 1, 1.f, 0, 1.0, acc, st);
}

extern "C" int m2t_consistency_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, int scale_factor,
                                           long long x_image_stride, int x_row_stride, float data_range, int clamp, double eps, double scale,
                                           float* gx_add, float* loss_out, double* stats_out, int accumulate, void* scratch, void* stream) {
  const char* const shape = cons_shape_refusal(B, C, H, W, scale_factor);
  const char* const more = (!(eps >= 0.0) || !isfinite(eps)) ? "eps must be a finite number >= 0" :
                           !isfinite(scale) ? "scale must be finite" : nullptr;
  if (int rc = loss_tensor_check(__func__, x, y, loss_out, scratch, C, shape ? 1 : H * scale_factor, shape ? 1 : W * scale_factor,
                                 x_image_stride, x_row_stride, data_range, shape, more))
    return rc;
  return launch_consistency_loss(x, y, B, C, H, W, scale_factor, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, eps, scale,
                                 gx_add, loss_out, stats_out, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}

extern "C" int m2t_back_project_f32(float* sr, const float* lr, int B, int C, int H, int W, int scale_factor, float data_range, double beta,
                                    int update, double* stats_out, void* scratch, void* stream) {
  if (!sr || !lr || !scratch) return m2t_set_error_at(M2T_ERR_ARG, __func__, "null argument");
  if (const char* r = cons_shape_refusal(B, C, H, W, scale_factor)) return m2t_set_error_at(M2T_ERR_ARG, __func__, r);
  if (!(data_range > 0.f) || !isfinite(data_range)) return m2t_set_error_at(M2T_ERR_ARG, __func__, "data_range must be a finite number > 0");
  if (!isfinite(beta) || !(beta > 0.0) || !(beta < 2.0))
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "beta must be a finite number inside (0, 2)");
  ConsLayout L;
  if (!cons_layout(B, C, H, W, scale_factor, L)) return m2t_set_error_at(M2T_ERR_ARG, __func__, "unsupported shape");
  hipStream_t st = (hipStream_t)stream;
  double* const sc = (double*)scratch;
  const int s = scale_factor;
  const long long img = (long long)C * H * s * W * s;
  int rc = s == 2 ? launch_down<2>(sr, img, W * s, C, lr, H, W, data_range, 1, 0.0, 1, L, sc, st) :
           s == 3 ? launch_down<3>(sr, img, W * s, C, lr, H, W, data_range, 1, 0.0, 1, L, sc, st) :
                    launch_down<4>(sr, img, W * s, C, lr, H, W, data_range, 1, 0.0, 1, L, sc, st);
  if (rc) return rc;
  if (stats_out && (rc = launch_finish(L, H, W, sc, 0.0, 0, nullptr, stats_out, st))) return rc;
  if (!update) return 0;
  return s == 2 ? launch_update<2>(sc + L.plane, sr, H, W, L.planes, data_range, beta, st) :
         s == 3 ? launch_update<3>(sc + L.plane, sr, H, W, L.planes, data_range, beta, st) :
                  launch_update<4>(sc + L.plane, sr, H, W, L.planes, data_range, beta, st);
}
