// k_gmsd_loss.hip -- the gradient-magnitude-similarity-deviation loss term (Xue et al. 2014; piq.GMSDLoss) with its gradient
// (include/m2t_gmsd.h has the definition; the reference scores every model by GMSD, test.py:95-122).
//
//   per image: u = the 2 x 2 average of luminance(clamp(x)) / R, v likewise of y (never clamped);  the zero-padded Prewitt pair,
//   differences first;  m, m' the gradient magnitudes;  d = 1 - s = (m - m')^2 / (m^2 + m'^2 + T);  GMSD_b = sqrt(var(d));
//   value = scale * sum_b GMSD_b.
//
// The gradient of every cell needs mean(d) and GMSD_b of the WHOLE image: two phases, coupled through a per-image record in device memory.
//   phase 1   one workgroup per 32 x 32 tile of the pooled map (m2t_gmsd_tile.h: value_tile): u and v of the tile plus halo in LDS,
//             the tile's sums of d and d^2.
//   record    one workgroup per image folds the partial sums in tile order: sum d, sum d^2, GMSD_b, scale / (n GMSD_b) (0 when GMSD_b
//             is 0); then one workgroup folds scale * sum_b GMSD_b into the loss.
//   phase 2   (only with a destination) the tile recomputes u and v on the tile plus 2, forms (a_x, a_y) on the tile plus 1, applies
//             the transposed Prewitt pair and adds 0.25 w_ch / R times the result to the 2 x 2 pixels x C channels the clamp lets
//             through, with ONE fp32 rounding.  A workgroup whose image has coefficient 0 returns at once.
// Each output element is written by exactly one thread, no atomics, fixed-order sums: two runs are bit-identical.
#include "m2t_common.h"
#include "m2t_kernels.h"
#include "m2t_gmsd_tile.h"
#include "../../include/m2t_gmsd.h"
#include <math.h>
#include <stdint.h>

namespace {

using namespace gmsd_tile;

constexpr int REC_SD = 0, REC_SD2 = 1, REC_GMSD = 2, REC_COEF = 3, REC = 4;      // the record of one image, in doubles

struct GmsdLayout { int hp, wp, ty, tx; size_t rec, part, total; };      // offsets and total in doubles

bool gmsd_layout(int B, int C, int H, int W, GmsdLayout& L) {
  if (B < 1 || B > 65535 || (C != 1 && C != 3) || H < 2 || W < 2) return false;
  L.hp = (H + 1) / 2; L.wp = (W + 1) / 2;
  L.ty = (L.hp + TP - 1) / TP; L.tx = (L.wp + TP - 1) / TP;
  if (L.ty > 65535) return false;
  L.rec = 0;
  L.part = (size_t)B * REC;
  L.total = L.part + (size_t)B * L.ty * L.tx * 2;
  return true;
}

__device__ __forceinline__ Src image_of(Src s, long long img_x, long long img_y, int b) {
  s.x += (long long)b * img_x;
  s.y += (long long)b * img_y;
  return s;
}

// Phase 1: grid (tiles_x, tiles_y, B); partial [B][tiles_y][tiles_x][2] = the tile's sums of d and d^2.
__global__ __launch_bounds__(256) void gmsd_value_kernel(Src src, long long img_x, long long img_y, int H, int W, int hp, int wp,
                                                         double* __restrict__ partial) {
  __shared__ __align__(16) unsigned char smem[SMEM_VALUE];
  const Src s = image_of(src, img_x, img_y, blockIdx.z);
  double sd, sd2;
  value_tile(smem, s, H, W, hp, wp, blockIdx.y * TP, blockIdx.x * TP, sd, sd2);
  if (threadIdx.x == 0) {
    double* const p = partial + (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    p[0] = sd; p[1] = sd2;
  }
}

// One workgroup per image: sum d, sum d^2, GMSD_b and the coefficient of phase 2.  Fixed order.
__global__ __launch_bounds__(256) void gmsd_record_kernel(const double* __restrict__ partial, int nt, double n, double scale,
                                                          double* __restrict__ rec, double* __restrict__ per_image_out) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  const double* const p = partial + (long long)b * nt * 2;
  double a = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < nt; i += 256) { a += p[2 * i]; q += p[2 * i + 1]; }
  const double sd = moment_tile::block_sum<256>(a, red);
  const double sd2 = moment_tile::block_sum<256>(q, red);
  if (threadIdx.x != 0) return;
  const double mean = sd / n;
  const double g = sqrt(fmax(sd2 / n - mean * mean, 0.0));
  double* const r = rec + (long long)b * REC;
  r[REC_SD] = sd; r[REC_SD2] = sd2; r[REC_GMSD] = g; r[REC_COEF] = g > 0.0 ? scale / (n * g) : 0.0;
  if (per_image_out) per_image_out[b] = g;
}

// Phase 2: grid (tiles_x, tiles_y, B); gx has x's strides.
__global__ __launch_bounds__(256) void gmsd_grad_kernel(Src src, long long img_x, long long img_y, int H, int W, int hp, int wp, double n,
                                                        const double* __restrict__ rec, float* __restrict__ gx) {
  __shared__ __align__(16) unsigned char smem[SMEM_GRAD];
  const int b = blockIdx.z;
  const double coef = rec[(long long)b * REC + REC_COEF];
  if (coef == 0.0) return;                                     // GMSD_b = 0 (identical images, a 1 x 1 map): nothing is written
  const Src s = image_of(src, img_x, img_y, b);
  grad_tile(smem, s, H, W, hp, wp, blockIdx.y * TP, blockIdx.x * TP, coef, rec[(long long)b * REC + REC_SD] / n,
            gx + (long long)b * img_x);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

size_t gmsd_loss_scratch_bytes(int B, int C, int H, int W) {
  GmsdLayout L;
  return gmsd_layout(B, C, H, W, L) ? sizeof(double) * L.total : 0;
}

bool gmsd_loss_size_supported(int H, int W) { return H >= 2 && W >= 2; }

// the one device routine behind m2t_gmsd_loss_tensor and m2t_gmsd_loss (arguments checked by the callers)
int launch_gmsd_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                     double scale, float* gx_add, float* loss_out, double* per_image_out, int accumulate, void* scratch, hipStream_t st) {
  GmsdLayout L;
  if (!gmsd_layout(B, C, H, W, L)) return m2t_set_error(M2T_ERR_ARG, "m2t_gmsd_loss: unsupported shape");
  const long long xs_ch = xs_img / C;
  Src s;
  s.x = x; s.y = y; s.xs_ch = xs_ch; s.xs_row = xs_row; s.ys_ch = (long long)H * W; s.ys_row = W; s.C = C; s.R = R; s.clamp = clamp;
  // 16-byte pieces: every row of every channel of every image must start on a 16-byte boundary, in x and in the destination alike
  s.vec_x = aligned16(x) && (!gx_add || aligned16(gx_add)) && xs_row % 4 == 0 && xs_ch % 4 == 0 && xs_img % 4 == 0;
  s.vec_y = aligned16(y) && W % 4 == 0;
  s.iR = 1.0 / (double)R;
  double* const sc = (double*)scratch;
  const long long img_y = (long long)C * H * W;
  const double n = (double)L.hp * (double)L.wp;
  const dim3 grid(L.tx, L.ty, B);
  gmsd_value_kernel<<<grid, NT, 0, st>>>(s, xs_img, img_y, H, W, L.hp, L.wp, sc + L.part);
  M2T_LAUNCH_CHECK();
  gmsd_record_kernel<<<B, 256, 0, st>>>(sc + L.part, L.ty * L.tx, n, scale, sc + L.rec, per_image_out);
  M2T_LAUNCH_CHECK();
  if (int rc = launch_loss_finish(sc + L.rec + REC_GMSD, B, REC, 0, scale, accumulate, loss_out, st)) return rc;      // sum_b GMSD_b
  if (!gx_add) return 0;
  gmsd_grad_kernel<<<grid, NT, 0, st>>>(s, xs_img, img_y, H, W, L.hp, L.wp, n, sc + L.rec, gx_add);
  M2T_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t m2t_gmsd_loss_scratch_bytes(int B, int C, int H, int W) { return gmsd_loss_scratch_bytes(B, C, H, W); }

extern "C" int m2t_gmsd_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                                    float data_range, int clamp, double scale, float* gx_add, float* loss_out, double* per_image_out,
                                    int accumulate, void* scratch, void* stream) {
  const char* const shape = (B < 1 || B > 65535) ? "need 1 <= B <= 65535" :
                            (C != 1 && C != 3) ? "C must be 1 or 3 (luminance of a grey or an RGB image)" :
                            !gmsd_loss_size_supported(H, W) ? "H and W must be at least 2 (one 2 x 2 cell)" :
                            ((H + 1) / 2 + TP - 1) / TP > 65535 ? "H is too large (at most 65535 tiles of 64 rows)" : nullptr;
  const char* const more = !isfinite(scale) ? "scale must be finite" : nullptr;
  if (int rc = loss_tensor_check(__func__, x, y, loss_out, scratch, C, H, W, x_image_stride, x_row_stride, data_range, shape, more))
    return rc;
  return launch_gmsd_loss(x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, scale, gx_add, loss_out,
                          per_image_out, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}
