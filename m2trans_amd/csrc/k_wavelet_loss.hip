// k_wavelet_loss.hip -- the wavelet-domain loss term: an L1 (or Charbonnier) on the detail bands of an undecimated (stationary,
// a-trous) 2-D wavelet transform of sr / R - hr / R with periodic borders, with its gradient; and the transform alone (m2t_swt2).
// include/m2t_wavelet.h has the definition; the model itself moves between its scales through a Haar DWT (m2t_haar.h).
//
//   forward   one launch per level j = 1 .. jmax (the highest level that carries a weight): a workgroup per 32 x 32 tile of one
//             (image, channel) plane (m2t_wavelet_tile.h: fwd_tile) stages its input with the level's reach -- the difference formed
//             from the fp32 pixels at level 1, the fp64 plane a_{j-1} after that -- and writes LL_j for the next level, w rho'(c)
//             of every weighted band as an fp64 plane, and the tile's sum of rho(c) per weighted band.
//   finish    one workgroup folds the partial sums band by band in tile order: per_band_out, then scale * sum_band w S.
//   backward  (only with a destination) one launch per level j = jmax .. 1 (bwd_tile): the transposed column passes of abar_j and
//             the psi planes, the transposed row passes, abar_{j-1}; level 1 adds scale / R * abar_0 into the destination through
//             the clamp mask with ONE fp32 rounding.
// A band of weight 0 costs no rho, no plane and no adjoint pass.  Each output element is written by exactly one thread, no atomics,
// fixed-order sums: two runs are bit-identical, and nothing read from the scratch was not written by the same call.
#include "m2t_common.h"
#include "m2t_kernels.h"
#include "m2t_wavelet_tile.h"
#include "../../include/m2t_wavelet.h"
#include <math.h>
#include <stdint.h>

namespace {

using namespace wavelet_tile;

struct WaveletLayout { int nb, ty, tx; size_t n, items, a[2], psi, part, total; };      // offsets and total in doubles

bool wavelet_layout(int B, int C, int H, int W, int levels, int taps, WaveletLayout& L) {
  if (!wavelet_shape_refusal(B, C, H, W, levels, taps)) {
    L.nb = 3 * levels + 1;
    L.ty = (H + TH - 1) / TH; L.tx = (W + TW - 1) / TW;
    L.n = (size_t)B * C * H * W;
    L.items = (size_t)B * C * L.ty * L.tx;
    L.a[0] = 0; L.a[1] = L.n;
    L.psi = 2 * L.n;
    L.part = L.psi + (size_t)L.nb * L.n;
    L.total = L.part + (size_t)L.nb * L.items;
    return true;
  }
  return false;
}

// what one forward level does for every plane; k = 0 LH, 1 HL, 2 HH, 3 LL
struct FwdLevel {
  int gb[4];             // the band's index among the 3 J + 1, or -1 (LL below the last level)
  double w[4];           // the loss: the band's weight (0: no rho, no psi)
  double eps;
  float* out; int nb;    // the transform alone: [B*C][nb][H][W] fp32, or nullptr
  double* psi;           // [nb][B*C][H][W] fp64, or nullptr (value only)
  double* a_out;         // [B*C][H][W] fp64, or nullptr (the last level)
  double* partial;       // [nb][items]
  int vec_f, vec_d;
};

template <bool FIRST, int HM>
__global__ __launch_bounds__(256) void wavelet_fwd_kernel(Src s, long long xs_img, int C, const double* __restrict__ a_in, int H, int W,
                                                          int dil, Filt f, FwdLevel lv) {
  __shared__ __align__(16) unsigned char smem[Geo<HM>::SMEM];
  const int z = blockIdx.z;
  const long long hw = (long long)H * W, n = hw * gridDim.z;
  FwdOut o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool on = lv.gb[k] >= 0;
    o.band[k] = lv.out && on ? lv.out + ((long long)z * lv.nb + lv.gb[k]) * hw : nullptr;
    o.w[k] = on && !lv.out ? lv.w[k] : 0.0;
    o.psi[k] = lv.psi && o.w[k] > 0.0 ? lv.psi + lv.gb[k] * n + z * hw : nullptr;
  }
  o.a_out = lv.a_out ? lv.a_out + z * hw : nullptr;
  o.eps = lv.eps; o.vec_f = lv.vec_f; o.vec_d = lv.vec_d;
  double sum[4];
  if (FIRST) {
    DiffSource src;
    src.s = s; src.W = W;
    src.s.x += (long long)(z / C) * xs_img + (long long)(z % C) * s.xs_ch;
    if (s.y) src.s.y += z * hw;
    fwd_tile<HM>(smem, src, H, W, blockIdx.y * TH, blockIdx.x * TW, dil, f, o, sum);
  } else {
    const PlaneSource src{a_in + z * hw, W, lv.vec_d};
    fwd_tile<HM>(smem, src, H, W, blockIdx.y * TH, blockIdx.x * TW, dil, f, o, sum);
  }
  if (threadIdx.x == 0) {
    const long long items = (long long)gridDim.x * gridDim.y * gridDim.z;
    const long long item = ((long long)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (o.w[k] > 0.0) lv.partial[lv.gb[k] * items + item] = sum[k];
  }
}

struct BandWeights { double w[MAXB]; };

// One workgroup: S_band = the partial sums of the band in tile order, per_band_out, loss = (accumulate ? loss : 0) +
// (float)(scale * sum_band w_band S_band), the bands ascending from 0.0.  A band of weight 0 has no partial sums: S = 0.
__global__ __launch_bounds__(256) void wavelet_finish_kernel(const double* __restrict__ partial, long long items, int nb, BandWeights bw,
                                                             double scale, int accumulate, float* __restrict__ loss,
                                                             double* __restrict__ per_band_out) {
  __shared__ double red[4];
  double total = 0.0;
#pragma unroll
  for (int b = 0; b < MAXB; ++b) {
    if (b < nb) {
      double S = 0.0;
      if (bw.w[b] > 0.0) {
        const double* const p = partial + (long long)b * items;
        double a = 0.0;
        for (long long i = threadIdx.x; i < items; i += 256) a += p[i];
        S = block_sum<256>(a, red);
        __syncthreads();
        total = total + bw.w[b] * S;
      }
      if (per_band_out && threadIdx.x == 0) per_band_out[b] = S;
    }
  }
  if (threadIdx.x == 0) {
    const float v = (float)(scale * total);
    loss[0] = accumulate ? loss[0] + v : v;
  }
}

struct BwdLevel { const double* abar; const double* lh; const double* hl; const double* hh; double* a_out; int vec_d; };

template <bool LAST, int HM>
__global__ __launch_bounds__(256) void wavelet_bwd_kernel(BwdLevel lv, int H, int W, int dil, Filt f, GradDst g, long long xs_img,
                                                          long long xs_ch, int C) {
  __shared__ __align__(16) unsigned char smem[Geo<HM>::SMEM];
  const int z = blockIdx.z;
  const long long off = (long long)z * H * W;
  BwdIn in;
  in.abar = lv.abar ? lv.abar + off : nullptr;
  in.lh = lv.lh ? lv.lh + off : nullptr;
  in.hl = lv.hl ? lv.hl + off : nullptr;
  in.hh = lv.hh ? lv.hh + off : nullptr;
  in.vec = lv.vec_d;
  if (LAST) {
    const long long o = (long long)(z / C) * xs_img + (long long)(z % C) * xs_ch;
    g.x += o; g.gx += o;
  }
  bwd_tile<LAST, HM>(smem, in, H, W, blockIdx.y * TH, blockIdx.x * TW, dil, f, LAST ? nullptr : lv.a_out + off, lv.vec_d, g);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

const char* wavelet_shape_refusal(int B, int C, int H, int W, int levels, int taps) {
  if (levels < 1 || levels > MAXJ) return "levels must be 1, 2 or 3";
  if (taps < 2 || taps > MAXL) return "the filters must have 2 to 8 taps";
  if (C != 1 && C != 3) return "C must be 1 or 3";
  if (B < 1 || (long long)B * C > 65535) return "need 1 <= B * C <= 65535";
  const int need = ((taps - 1) << (levels - 1)) + 1;
  if (H < need || W < need) return "H and W must be at least (taps - 1) * 2^(levels - 1) + 1 (a tap index wraps at most once)";
  if ((H + TH - 1) / TH > 65535) return "H is too large (at most 65535 tiles of 32 rows)";
  return nullptr;
}

const char* wavelet_filter_refusal(const double* lo, const double* hi, int taps, int levels, const double* band_weights, double eps) {
  if (levels < 1 || levels > MAXJ) return "levels must be 1, 2 or 3";
  if (taps < 2 || taps > MAXL) return "the filters must have 2 to 8 taps";
  for (int k = 0; k < taps; ++k)
    if (!isfinite(lo[k]) || !isfinite(hi[k])) return "the filter taps must be finite";
  if (band_weights) {
    bool any = false;
    for (int b = 0; b < 3 * levels + 1; ++b) {
      if (!isfinite(band_weights[b]) || band_weights[b] < 0.0) return "the band weights must be finite and >= 0";
      any = any || band_weights[b] > 0.0;
    }
    if (!any) return "the band weights must not all be 0";
  }
  if (!isfinite(eps) || eps < 0.0) return "eps must be finite and >= 0";
  return nullptr;
}

size_t wavelet_loss_scratch_bytes(int B, int C, int H, int W, int levels, int taps) {
  WaveletLayout L;
  return wavelet_layout(B, C, H, W, levels, taps, L) ? sizeof(double) * L.total : 0;
}

// the one device routine behind m2t_swt2, m2t_wavelet_loss_tensor and m2t_wavelet_loss (arguments checked by the callers).
// swt_out != nullptr: the transform of x alone (y, the weights, the loss and the gradient unused).
int launch_wavelet_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                        double scale, const double* lo, const double* hi, int taps, int levels, const double* band_weights, double eps,
                        float* swt_out, float* gx_add, float* loss_out, double* per_band_out, int accumulate, void* scratch,
                        hipStream_t st) {
  WaveletLayout L;
  if (!wavelet_layout(B, C, H, W, levels, taps, L)) return m2t_set_error(M2T_ERR_ARG, "m2t_wavelet_loss: unsupported shape");
  Filt f;
  for (int k = 0; k < MAXL; ++k) { f.lo[k] = k < taps ? lo[k] : 0.0; f.hi[k] = k < taps ? hi[k] : 0.0; }
  f.taps = taps;
  BandWeights bw;
  for (int b = 0; b < MAXB; ++b) bw.w[b] = swt_out || b >= L.nb ? 0.0 : band_weights ? band_weights[b] : b < 3 * levels ? 1.0 : 0.0;
  int jmax = levels;                                           // the highest level that carries a weight: nothing above it is computed
  if (!swt_out)
    while (jmax > 1 && !(bw.w[3 * (jmax - 1)] > 0.0 || bw.w[3 * (jmax - 1) + 1] > 0.0 || bw.w[3 * (jmax - 1) + 2] > 0.0 ||
                         (jmax == levels && bw.w[3 * levels] > 0.0)))
      --jmax;
  const long long xs_ch = xs_img / C;
  Src s;
  s.x = x; s.y = y; s.xs_ch = xs_ch; s.xs_row = xs_row; s.R = R; s.clamp = clamp; s.iR = 1.0 / (double)R;
  // 16-byte pieces: every row of every plane must start on a 16-byte boundary, in x and in the destination alike
  s.vec_x = aligned16(x) && (!gx_add || aligned16(gx_add)) && xs_row % 4 == 0 && xs_ch % 4 == 0 && xs_img % 4 == 0;
  s.vec_y = y && aligned16(y) && W % 4 == 0;
  double* const sc = (double*)scratch;
  const int vec_d = aligned16(scratch) && W % 2 == 0;
  const dim3 grid(L.tx, L.ty, B * C);
  for (int j = 1; j <= jmax; ++j) {
    FwdLevel lv;
    for (int k = 0; k < 3; ++k) lv.gb[k] = 3 * (j - 1) + k;
    lv.gb[3] = j == levels ? 3 * levels : -1;
    for (int k = 0; k < 4; ++k) lv.w[k] = lv.gb[k] >= 0 ? bw.w[lv.gb[k]] : 0.0;
    lv.eps = eps;
    lv.out = swt_out; lv.nb = L.nb;
    lv.psi = gx_add ? sc + L.psi : nullptr;
    lv.a_out = j < jmax ? sc + L.a[j & 1] : nullptr;
    lv.partial = sc + L.part;
    lv.vec_f = swt_out && aligned16(swt_out) && W % 4 == 0;
    lv.vec_d = vec_d;
    const int dil = 1 << (j - 1);
    const double* const a_in = sc + L.a[(j - 1) & 1];
    if (small_reach(taps, dil)) {                              // (the variant with the smaller staged region: four workgroups per CU)
      if (j == 1) wavelet_fwd_kernel<true, HM_SMALL><<<grid, NT, 0, st>>>(s, xs_img, C, nullptr, H, W, dil, f, lv);
      else wavelet_fwd_kernel<false, HM_SMALL><<<grid, NT, 0, st>>>(s, xs_img, C, a_in, H, W, dil, f, lv);
    } else {
      if (j == 1) wavelet_fwd_kernel<true, HM_BIG><<<grid, NT, 0, st>>>(s, xs_img, C, nullptr, H, W, dil, f, lv);
      else wavelet_fwd_kernel<false, HM_BIG><<<grid, NT, 0, st>>>(s, xs_img, C, a_in, H, W, dil, f, lv);
    }
    M2T_LAUNCH_CHECK();
  }
  if (swt_out) return 0;
  wavelet_finish_kernel<<<1, 256, 0, st>>>(sc + L.part, (long long)L.items, L.nb, bw, scale, accumulate, loss_out, per_band_out);
  M2T_LAUNCH_CHECK();
  if (!gx_add) return 0;
  GradDst g;
  g.x = x; g.gx = gx_add; g.xs_row = xs_row; g.R = R; g.clamp = clamp; g.vec = s.vec_x; g.coef = scale * s.iR;
  for (int j = jmax; j >= 1; --j) {
    const auto psi = [&](int b) -> const double* { return bw.w[b] > 0.0 ? sc + L.psi + (size_t)b * L.n : nullptr; };
    BwdLevel lv;
    lv.abar = j == levels ? psi(3 * levels) : j == jmax ? nullptr : sc + L.a[j & 1];
    lv.lh = psi(3 * (j - 1)); lv.hl = psi(3 * (j - 1) + 1); lv.hh = psi(3 * (j - 1) + 2);
    lv.a_out = sc + L.a[(j - 1) & 1];
    lv.vec_d = vec_d;
    const int dil = 1 << (j - 1);
    if (small_reach(taps, dil)) {
      if (j == 1) wavelet_bwd_kernel<true, HM_SMALL><<<grid, NT, 0, st>>>(lv, H, W, dil, f, g, xs_img, xs_ch, C);
      else wavelet_bwd_kernel<false, HM_SMALL><<<grid, NT, 0, st>>>(lv, H, W, dil, f, g, xs_img, xs_ch, C);
    } else {
      if (j == 1) wavelet_bwd_kernel<true, HM_BIG><<<grid, NT, 0, st>>>(lv, H, W, dil, f, g, xs_img, xs_ch, C);
      else wavelet_bwd_kernel<false, HM_BIG><<<grid, NT, 0, st>>>(lv, H, W, dil, f, g, xs_img, xs_ch, C);
    }
    M2T_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" size_t m2t_wavelet_loss_scratch_bytes(int B, int C, int H, int W, int levels, int taps) {
  return wavelet_loss_scratch_bytes(B, C, H, W, levels, taps);
}

extern "C" int m2t_swt2(const float* x, int B, int C, int H, int W, long long x_image_stride, int x_row_stride, const double* lo,
                        const double* hi, int taps, int levels, float* out, void* scratch, void* stream) {
  if (!x || !lo || !hi || !out || !scratch) return m2t_set_error_at(M2T_ERR_ARG, __func__, "null argument");
  if (const char* r = wavelet_filter_refusal(lo, hi, taps, levels, nullptr, 0.0)) return m2t_set_error_at(M2T_ERR_ARG, __func__, r);
  if (const char* r = wavelet_shape_refusal(B, C, H, W, levels, taps)) return m2t_set_error_at(M2T_ERR_ARG, __func__, r);
  if (x_row_stride < W || x_image_stride % C != 0 || x_image_stride / C < (long long)(H - 1) * x_row_stride + W)
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "strides of x do not hold a [C][H][W] image (channel stride = x_image_stride / C)");
  return launch_wavelet_loss(x, nullptr, B, C, H, W, x_image_stride, x_row_stride, 1.f, 0, 1.0, lo, hi, taps, levels, nullptr, 0.0, out,
                             nullptr, nullptr, nullptr, 0, scratch, (hipStream_t)stream);
}

extern "C" int m2t_wavelet_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride,
                                       int x_row_stride, float data_range, int clamp, double scale, const double* lo, const double* hi,
                                       int taps, int levels, const double* band_weights, double eps, float* gx_add, float* loss_out,
                                       double* per_band_out, int accumulate, void* scratch, void* stream) {
  if (!lo || !hi) return m2t_set_error_at(M2T_ERR_ARG, __func__, "null argument");
  const char* const filt = wavelet_filter_refusal(lo, hi, taps, levels, band_weights, eps);
  const char* const shape = filt ? filt : wavelet_shape_refusal(B, C, H, W, levels, taps);
  const char* const more = !isfinite(scale) ? "scale must be finite" : nullptr;
  if (int rc = loss_tensor_check(__func__, x, y, loss_out, scratch, C, H, W, x_image_stride, x_row_stride, data_range, shape, more))
    return rc;
  return launch_wavelet_loss(x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, scale, lo, hi, taps, levels,
                             band_weights, eps, nullptr, gx_add, loss_out, per_band_out, accumulate ? 1 : 0, scratch,
                             (hipStream_t)stream);
}
