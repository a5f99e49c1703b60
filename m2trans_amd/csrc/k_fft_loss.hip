// k_fft_loss.hip -- the frequency-domain loss term: an L1 on the coefficients of a 2-D real FFT, with its gradient (the reference
// imports torch.fft in losses.py:5 and models/M2Trans_network.py:8 and never calls it; the term is MIMO-UNet's
// F.l1_loss(view_as_real(rfft2(sr)), view_as_real(rfft2(hr))) next to the pixel loss).
//
//   per plane (sample, channel):  d = (clamp(pre, 0, R) - hr) / R,  D = s * rfft2(d)  (H x (W/2+1); s = 1 "backward", 1/sqrt(HW) "ortho"),
//   value = scale * sum (|Re D| + |Im D|)          (scale = weight / (2 * planes * H * (W/2+1)) for the mean),
//   d value / d pre(h, w) = scale * s / R * Re sum_ky sum_{kx <= W/2} (sign Re D + i sign Im D) e^{+2 pi i (ky h / H + kx w / W)},
//   sign(0) = 0; the imaginary part of the four self-conjugate bins (ky in {0, H/2}, kx in {0, W/2}) is exactly 0, sign 0.
//
// H and W are even, 8 .. 2048, of the form 2^a 3^b (x3 patches are 768 = 3 * 2^8 wide).  Three launches over one fp32 complex
// half spectrum [planes][H][W/2+1] in the caller's scratch (a plane does not fit in LDS):
//   1. fft_rows_fwd_kernel    forms d, transforms the rows (two real rows = one complex sequence), writes the half spectrum;
//   2. fft_cols_kernel        a strip of adjacent kx over all H: column transform, sum |Re| + |Im| into an fp64 partial, signs,
//                             the inverse-direction column transform of the signs without leaving LDS, back over the same scratch;
//   3. fft_rows_adj_kernel    the half-spectrum complex-to-real pass (no Hermitian doubling) and the add into the seed through
//                             the clamp mask: one fp32 rounding per gradient value.
// The arithmetic (Stockham stages of radix 4 / 2 / 3 in LDS, fp32 butterflies) is m2t_fft.h.  Twiddles: one table of the N-th roots
// per length, fp64 on the host, rounded once to fp32.  Partial sums are fp64, one per workgroup, folded by one workgroup in a
// fixed order: no atomics, two runs are bit-identical.
#include "m2t_common.h"
#include "m2t_kernels.h"
#include "m2t_fft.h"
#include "m2t_moment_tile.h"      // block_sum
#include "../../include/m2t_spectral.h"
#include <math.h>
#include <map>
#include <utility>
#include <vector>

namespace {

using namespace m2t_fft;
constexpr int NT = 256;

using moment_tile::block_sum;

// all stages of one transform on the sequences in a (b = the other ping-pong buffer); the caller has synchronised after filling a;
// returns the buffer that holds the result, synchronised
__device__ __forceinline__ float2* fft_run(float2* a, float2* b, int N, int ld, int nseq, const float2* __restrict__ tw, int inv) {
  int n = N, s = 1;
  while (n > 1) {
    const int r = next_radix(n);
    stage_any(r, a, b, N, ld, nseq, s, tw, inv, threadIdx.x, NT);
    __syncthreads();
    float2* const t = a; a = b; b = t;
    n /= r; s *= r;
  }
  return a;
}

// grid: ceil(npairs / nseq) workgroups; LDS 2 * nseq * W complex
__global__ __launch_bounds__(NT) void fft_rows_fwd_kernel(Image im, int nseq, const float2* __restrict__ tw, float2* __restrict__ spec) {
  extern __shared__ __align__(16) unsigned char smem[];
  float2* const a = (float2*)smem;
  float2* const b = a + nseq * im.W;
  rows_load(im, a, nseq, blockIdx.x, threadIdx.x, NT);
  __syncthreads();
  const float2* const z = fft_run(a, b, im.W, im.W, nseq, tw, 0);
  rows_write(im, z, spec, nseq, blockIdx.x, threadIdx.x, NT);
}

// grid (strips, planes); LDS 2 * sw * ld complex.  mode 0: the plain transform (values * scale stay in spec); 1: value only;
// 2: value and the adjoint column transform of the signs
__global__ __launch_bounds__(NT) void fft_cols_kernel(float2* __restrict__ spec, int H, int W, int sw, int ld, const float2* __restrict__ tw,
                                                      int mode, float scale, double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double red[NT / 64];
  float2* const a = (float2*)smem;
  float2* const b = a + sw * ld;
  const int Wh = W / 2 + 1, kx0 = blockIdx.x * sw;
  const long long plane = blockIdx.y;
  cols_load(spec, a, plane, H, Wh, kx0, sw, ld, threadIdx.x, NT);
  __syncthreads();
  float2* z = fft_run(a, b, H, ld, sw, tw, 0);
  const double acc = cols_mid(z, H, W, kx0, sw, ld, mode != 0, scale, threadIdx.x, NT);
  if (mode != 0) {
    const double t = block_sum<NT>(acc, red);              // (its barriers also close the signs)
    if (threadIdx.x == 0) partial[plane * gridDim.x + blockIdx.x] = t;
    if (mode == 1) return;
    z = fft_run(z, z == a ? b : a, H, ld, sw, tw, 1);
  } else {
    __syncthreads();
  }
  cols_write(spec, z, plane, H, Wh, kx0, sw, ld, threadIdx.x, NT);
}

__global__ __launch_bounds__(NT) void fft_rows_adj_kernel(Image im, int nseq, const float2* __restrict__ tw, const float2* __restrict__ spec,
                                                          double gcoef) {
  extern __shared__ __align__(16) unsigned char smem[];
  float2* const a = (float2*)smem;
  float2* const b = a + nseq * im.W;
  rowsadj_load(im, spec, a, nseq, blockIdx.x, threadIdx.x, NT);
  __syncthreads();
  const float2* const z = fft_run(a, b, im.W, im.W, nseq, tw, 1);
  rowsadj_add(im, z, gcoef, nseq, blockIdx.x, threadIdx.x, NT);
}

// The N-th roots of unity e^{-2 pi i j / N}, j < N: fp64 on the host, rounded once to fp32, uploaded ONCE per (calling thread,
// device, length) -- the one allocation this library makes on its own (a few KB per length; m2t_rfft2 has no scratch argument to
// hold it).  The cache is thread-local, as m2t_ensure_dynamic_lds's: no process-global mutable state.  The first call with a new
// length therefore synchronises (hipMemcpy) and must not sit inside a stream capture; later calls only launch.
int twiddles(int N, const float2** out) {
  static thread_local std::map<std::pair<int, int>, float2*> cache;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  auto it = cache.find({dev, N});
  if (it != cache.end()) { *out = it->second; return 0; }
  std::vector<float2> host((size_t)N);
  for (int j = 0; j < N; ++j) {
    // exact at the multiples of a quarter turn, where cos / sin of the rounded angle would leave 6e-17 in place of 0
    const double ang = -2.0 * M_PI * (double)j / (double)N;
    double c = cos(ang), s = sin(ang);
    if ((4 * j) % N == 0) { const int qd = 4 * j / N; c = qd == 0 ? 1.0 : (qd == 2 ? -1.0 : 0.0); s = qd == 1 ? -1.0 : (qd == 3 ? 1.0 : 0.0); }
    host[(size_t)j] = make_float2((float)c, (float)s);
  }
  float2* d = nullptr;
  e = hipMalloc((void**)&d, sizeof(float2) * (size_t)N);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  e = hipMemcpy(d, host.data(), sizeof(float2) * (size_t)N, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d); return m2t_set_hip_error(e, __FILE__, __LINE__); }
  cache[{dev, N}] = d;
  *out = d;
  return 0;
}

size_t spectrum_bytes(long long planes, int H, int W) { return sizeof(float2) * (size_t)planes * (size_t)H * (size_t)(W / 2 + 1); }

int launch_rows_fwd(const Image& im, const float2* twW, float2* spec, hipStream_t st) {
  const int nseq = rows_nseq(im.W);
  const int lds = (int)(2 * sizeof(float2)) * nseq * im.W;
  if (int rc = m2t_ensure_dynamic_lds((const void*)fft_rows_fwd_kernel, lds)) return rc;
  fft_rows_fwd_kernel<<<(unsigned)((im.npairs + nseq - 1) / nseq), NT, lds, st>>>(im, nseq, twW, spec);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_cols(float2* spec, long long planes, int H, int W, const float2* twH, int mode, float scale, double* partial, hipStream_t st) {
  const int sw = cols_strip(H), ld = cols_ld(H, sw), strips = (W / 2 + 1 + sw - 1) / sw;
  const int lds = (int)(2 * sizeof(float2)) * sw * ld;
  if (int rc = m2t_ensure_dynamic_lds((const void*)fft_cols_kernel, lds)) return rc;
  fft_cols_kernel<<<dim3(strips, (unsigned)planes), NT, lds, st>>>(spec, H, W, sw, ld, twH, mode, scale, partial);
  M2T_LAUNCH_CHECK();
  return 0;
}

float norm_scale(int norm, int H, int W) { return norm == 1 ? (float)(1.0 / sqrt((double)H * (double)W)) : 1.f; }

}  // namespace

bool fft_loss_size_supported(int H, int W) { return size_supported(H) && size_supported(W); }

size_t fft_loss_scratch_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || (long long)B * C > 65535 || !fft_loss_size_supported(H, W)) return 0;
  const int sw = cols_strip(H), strips = (W / 2 + 1 + sw - 1) / sw;
  return spectrum_bytes((long long)B * C, H, W) + sizeof(double) * (size_t)B * C * strips;
}

// the one device routine behind m2t_fft_loss_tensor and m2t_fft_loss (arguments checked by the callers)
int launch_fft_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp, int norm,
                    double scale, float* gx_add, float* loss_out, int accumulate, void* scratch, hipStream_t st) {
  const float2 *twW = nullptr, *twH = nullptr;
  if (int rc = twiddles(W, &twW)) return rc;
  if (int rc = twiddles(H, &twH)) return rc;
  const long long planes = (long long)B * C;
  const Image im{x, y, gx_add, C, H, W, xs_img, xs_img / C, xs_row, R, clamp, planes * (H / 2)};
  float2* const spec = (float2*)scratch;
  double* const partial = (double*)((char*)scratch + spectrum_bytes(planes, H, W));
  const int sw = cols_strip(H), strips = (W / 2 + 1 + sw - 1) / sw;
  const double s = norm == 1 ? 1.0 / sqrt((double)H * (double)W) : 1.0;
  if (int rc = launch_rows_fwd(im, twW, spec, st)) return rc;
  if (int rc = launch_cols(spec, planes, H, W, twH, gx_add ? 2 : 1, 1.f, partial, st)) return rc;
  if (gx_add) {
    const int nseq = rows_nseq(W);
    const int lds = (int)(2 * sizeof(float2)) * nseq * W;
    if (int rc = m2t_ensure_dynamic_lds((const void*)fft_rows_adj_kernel, lds)) return rc;
    fft_rows_adj_kernel<<<(unsigned)((im.npairs + nseq - 1) / nseq), NT, lds, st>>>(im, nseq, twW, spec, scale * s / (double)R);
    M2T_LAUNCH_CHECK();
  }
  return launch_loss_finish(partial, planes * strips, 1, 0, scale * s, accumulate, loss_out, st);
}

extern "C" size_t m2t_fft_loss_scratch_bytes(int B, int C, int H, int W) { return fft_loss_scratch_bytes(B, C, H, W); }

extern "C" int m2t_rfft2(const float* x, float* out, int planes, int H, int W, int norm, void* stream) {
  if (!x || !out) return m2t_set_error(M2T_ERR_ARG, "m2t_rfft2: null argument");
  if (planes < 1 || planes > 65535) return m2t_set_error(M2T_ERR_ARG, "m2t_rfft2: need 1 <= planes <= 65535");
  if (!fft_loss_size_supported(H, W))
    return m2t_set_error(M2T_ERR_ARG, "m2t_rfft2: H and W must be even, 8 .. 2048 and of the form 2^a * 3^b");
  if (norm != 0 && norm != 1) return m2t_set_error(M2T_ERR_ARG, "m2t_rfft2: norm must be 0 (backward) or 1 (ortho)");
  const float2 *twW = nullptr, *twH = nullptr;
  if (int rc = twiddles(W, &twW)) return rc;
  if (int rc = twiddles(H, &twH)) return rc;
  const Image im{x, nullptr, nullptr, 1, H, W, (long long)H * W, (long long)H * W, W, 1.f, 0, (long long)planes * (H / 2)};
  if (int rc = launch_rows_fwd(im, twW, (float2*)out, (hipStream_t)stream)) return rc;
  return launch_cols((float2*)out, planes, H, W, twH, 0, norm_scale(norm, H, W), nullptr, (hipStream_t)stream);
}

extern "C" int m2t_fft_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                                   float data_range, int clamp, int norm, double scale, float* gx_add, float* loss_out, int accumulate,
                                   void* scratch, void* stream) {
  const char* const shape = (B < 1 || C < 1 || (long long)B * C > 65535) ? "need 1 <= B * C <= 65535" :
                            !fft_loss_size_supported(H, W) ? "H and W must be even, 8 .. 2048 and of the form 2^a * 3^b" : nullptr;
  const char* const more = (norm != 0 && norm != 1) ? "norm must be 0 (backward) or 1 (ortho)" : !isfinite(scale) ? "scale must be finite" : nullptr;
  if (int rc = loss_tensor_check(__func__, x, y, loss_out, scratch, C, H, W, x_image_stride, x_row_stride, data_range, shape, more))
    return rc;
  return launch_fft_loss(x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, norm, scale, gx_add, loss_out,
                         accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}
