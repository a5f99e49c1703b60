// k_vgg.hip -- the kernels of the VGG19 feature loss (include/m2t_perceptual.h; host layer in m2t_vgg.hip).
//
// Activations are bf16 NHWC, weights bf16 (rounded once at load), accumulation fp32.
//
//   vgg_conv3x3_kernel   3 x 3, zero padding 1, stride 1, Cin and Cout multiples of 64: an implicit GEMM on v_mfma_f32_16x16x32_bf16.
//                        One workgroup (4 waves) owns 16 x 16 output pixels x 64 output channels; wave w owns rows 4w .. 4w + 3.  The k-loop
//                        walks Cin in chunks of 32: the 18 x 18 halo of the chunk and the chunk's 9 x 64 x 32 weights go to LDS once and
//                        are read by all nine taps.  The weights are the A operand (rows = output channels) and the pixels the B operand
//                        (columns = 16 pixels of one row), so that a lane ends with 4 consecutive output channels of one pixel: an 8-byte
//                        store.  Both operand reads are ds_read_b128 over 1 KB that the wave covers contiguously (lane (i, g) reads bytes
//                        64 i + 16 g of its row of 16 pixels / 16 channels): no bank conflict, no padding.  Edge tiles are predicated: halo
//                        pixels outside the image are zero, stores outside the image are dropped.
//                        EPI 0 (forward): bias, ReLU, one rounding.  EPI 1 (data gradient: the same GEMM on flipped, transposed weights):
//                        + the tap seed gscale * rho'(a - f_y) in fp32, times the ReLU mask a > 0 of the producing layer's saved output,
//                        one rounding.
//   vgg_first_*          conv1_1 (K = 27: VALU) with the normalisation and clamp fused, and its 64 -> 3 data gradient into the caller's
//                        fp32 buffer.
//   vgg_pool_*           2 x 2 stride-2 max pool (floor sizes) and its gradient (first maximum in row-major order, as torch).
//   vgg_tap_*            the distance of one tap: fp64 partial sums per block, folded in a fixed order; the seed of relu5_1.
// No atomics; every output element is written by exactly one thread.
#include "m2t_kernels.h"
#include "m2t_pixel_loss.h"

namespace {

constexpr int TP = 16;                 // output tile: TP x TP pixels
constexpr int HP = TP + 2;             // halo side
constexpr int KC = 32;                 // Cin per chunk = the k of one MFMA
constexpr int NT = 64;                 // Cout per workgroup

__device__ __forceinline__ float seed_factor(const M2TPixelLoss& s, float a, float fy) {
  float term;
  return s.gscale * m2t_pixel_loss_eval(s.kind, a - fy, s.param, s.f0, s.f1, term);
}

template <int EPI>
__global__ __launch_bounds__(256) void vgg_conv3x3_kernel(const bf16_t* __restrict__ in, const bf16_t* __restrict__ wpk, bf16_t* __restrict__ out,
                                                          int H, int W, int Cin, int Cout, int tiles_x, const float* __restrict__ bias,
                                                          const bf16_t* __restrict__ mask, const bf16_t* __restrict__ ytap, M2TPixelLoss sd) {
  __shared__ __attribute__((aligned(16))) bf16_t s_in[HP * HP * KC];
  __shared__ __attribute__((aligned(16))) bf16_t s_w[9 * NT * KC];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, g = lane >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * TP, x0 = tx * TP, ct = blockIdx.y, n = blockIdx.z;
  const int nchunk = Cin / KC;
  const bf16_t* inb = in + (long long)n * H * W * Cin;
  const bool live = y0 + 4 * wv < H;   // wave-uniform: a wave whose four rows lie under the image only helps with the copies

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[a][r] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int ch = 0; ch < nchunk; ++ch) {
    if (ch) __syncthreads();
    for (int v = tid; v < HP * HP * 4; v += 256) {
      const int pix = v >> 2, q = v & 3, hy = pix / HP, hx = pix - hy * HP;
      const int gy = y0 + hy - 1, gx = x0 + hx - 1;
      Frag8<bf16_t> f = frag_zero<bf16_t>();
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) f = load8(inb + ((long long)gy * W + gx) * Cin + ch * KC + q * 8);
      store8(&s_in[pix * KC + q * 8], f);
    }
    const bf16_t* wsrc = wpk + ((long long)ct * nchunk + ch) * (9 * NT * KC);
    for (int v = tid; v < 9 * NT * KC / 8; v += 256) store8(&s_w[v * 8], load8(wsrc + v * 8));
    __syncthreads();
    if (live) {
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          Frag8<bf16_t> a[4], b[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) a[c] = load8(&s_w[(((dy * 3 + dx) * NT) + c * 16 + i) * KC + g * 8]);
#pragma unroll
          for (int r = 0; r < 4; ++r) b[r] = load8(&s_in[((4 * wv + r + dy) * HP + i + dx) * KC + g * 8]);
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) mma16(acc[c][r], a[c], b[r]);
        }
    }
  }
  if (!live) return;
  const int x = x0 + i;
  if (x >= W) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int y = y0 + 4 * wv + r;
    if (y >= H) continue;
    const long long o = (((long long)n * H + y) * W + x) * Cout + ct * NT + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v[4];
      if (EPI == 0) {
        float b4[4];
        load4(bias + ct * NT + c * 16 + 4 * g, b4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[c][r][e] + b4[e], 0.f);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[c][r][e];
        if (mask) {
          float a4[4];
          load4(mask + o + c * 16, a4);
          if (ytap) {
            float f4[4];
            load4(ytap + o + c * 16, f4);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] + seed_factor(sd, a4[e], f4[e]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = a4[e] > 0.f ? v[e] : 0.f;
        }
      }
      store4(out + o + c * 16, v);
    }
  }
}

// torch [Cout][Cin][3][3] fp32 -> [Cout' / 64][Cin' / 32][9][64][32] bf16.  flip = 0: the forward operand (Cout' = Cout, Cin' = Cin).
// flip = 1: the data gradient's (Cout' = Cin, Cin' = Cout, w'[co'][ci'][t'] = w[ci'][co'][8 - t']).
__global__ void vgg_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst, int Cout, int Cin, int flip) {
  const long long total = (long long)Cout * Cin * 9;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cinp = flip ? Cout : Cin;
  const int nchunk = cinp / KC;
  long long t = idx;
  const int ci = (int)(t % KC); t /= KC;
  const int co = (int)(t % NT); t /= NT;
  const int tap = (int)(t % 9); t /= 9;
  const int ch = (int)(t % nchunk); t /= nchunk;
  const int cot = (int)t;
  const int cop = cot * NT + co, cip = ch * KC + ci;
  const float v = flip ? w[((long long)cip * Cin + cop) * 9 + (8 - tap)] : w[((long long)cop * Cin + cip) * 9 + tap];
  dst[idx] = (bf16_t)v;
}

// conv1_1's weights [64][3][3][3] -> fp32 [27][64] (tap-major, t = (dy * 3 + dx) * 3 + ci), each value rounded to bf16 first
__global__ void vgg_pack_first_kernel(const float* __restrict__ w, float* __restrict__ dst) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 27 * 64) return;
  const int co = idx & 63, t = idx >> 6, ci = t % 3, tap = t / 3;
  dst[idx] = (float)(bf16_t)w[(co * 3 + ci) * 9 + tap];
}

__device__ __forceinline__ float vgg_mean(int c) { return c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f); }
__device__ __forceinline__ float vgg_std(int c) { return c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f); }

// conv1_1 + ReLU on (c(x) / R - mean) / std; one thread per pixel, all 64 output channels.  chs = 0 repeats one channel to three.
__global__ __launch_bounds__(256) void vgg_first_fwd_kernel(const float* __restrict__ x, long long img, long long chs, int row, float R, int clamp,
                                                            const float* __restrict__ w0, const float* __restrict__ bias,
                                                            bf16_t* __restrict__ out, int H, int W) {
  const int p = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (p >= H * W) return;
  const int y = p / W, xx = p - y * W;
  float acc[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) acc[k] = bias[k];
  const float* xb = x + (long long)n * img;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int gy = y + dy - 1, gx = xx + dx - 1;
      const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        float a = 0.f;
        if (ok) {
          float v = xb[ci * chs + (long long)gy * row + gx];
          if (clamp) v = fminf(fmaxf(v, 0.f), R);
          a = (v / R - vgg_mean(ci)) / vgg_std(ci);
        }
        const float* wr = w0 + ((dy * 3 + dx) * 3 + ci) * 64;
#pragma unroll
        for (int k = 0; k < 64; ++k) acc[k] = fmaf(a, wr[k], acc[k]);
      }
    }
  bf16_t* o = out + ((long long)n * H * W + p) * 64;
#pragma unroll
  for (int k8 = 0; k8 < 8; ++k8) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fmaxf(acc[k8 * 8 + e], 0.f);
    store8f(o + k8 * 8, v);
  }
}

// the 64 -> 3 data gradient of conv1_1, through the normalisation (1 / (std R)) and the clamp mask, ADDED into gx (x's strides).
// g: the gradient at conv1_1's output, bf16 [N][H][W][64].  With chs = 0 the three channels' gradients are summed into the one plane.
__global__ __launch_bounds__(256) void vgg_first_bwd_kernel(const bf16_t* __restrict__ g, const float* __restrict__ w0, const float* x,
                                                            float* gx, long long img, long long chs, int row, float R, int clamp,
                                                            int H, int W) {
  const int p = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (p >= H * W) return;
  const int y = p / W, xx = p - y * W;
  float acc[3] = {0.f, 0.f, 0.f};
  const bf16_t* gb = g + (long long)n * H * W * 64;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int qy = y - (dy - 1), qx = xx - (dx - 1);
      if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
      const bf16_t* gp = gb + ((long long)qy * W + qx) * 64;
      const float* wr = w0 + (dy * 3 + dx) * 3 * 64;
#pragma unroll
      for (int k8 = 0; k8 < 8; ++k8) {
        float v[8];
        load8f(gp + k8 * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int ci = 0; ci < 3; ++ci) acc[ci] = fmaf(v[e], wr[ci * 64 + k8 * 8 + e], acc[ci]);
      }
    }
  const long long base = (long long)n * img + (long long)y * row + xx;
  if (chs == 0) {
    const float xv = x[base];
    if (clamp && !(xv >= 0.f && xv <= R)) return;
    const float s = (acc[0] / (vgg_std(0) * R) + acc[1] / (vgg_std(1) * R)) + acc[2] / (vgg_std(2) * R);
    gx[base] = gx[base] + s;
    return;
  }
#pragma unroll
  for (int ci = 0; ci < 3; ++ci) {
    const long long o = base + ci * chs;
    const float xv = x[o];
    if (clamp && !(xv >= 0.f && xv <= R)) continue;
    gx[o] = gx[o] + acc[ci] / (vgg_std(ci) * R);
  }
}

// 2 x 2 stride-2 max pool, floor sizes; one thread per output pixel and 8 channels
__global__ void vgg_pool_fwd_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int N, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, c8 = C / 8;
  const long long total = (long long)N * Ho * Wo * c8;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  long long t = idx;
  const int c = (int)(t % c8) * 8; t /= c8;
  const int ox = (int)(t % Wo); t /= Wo;
  const int oy = (int)(t % Ho);
  const int n = (int)(t / Ho);
  const bf16_t* p = in + (((long long)n * H + 2 * oy) * W + 2 * ox) * C + c;
  float a[8], b[8];
  load8f(p, a);
  load8f(p + C, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = fmaxf(a[e], b[e]);
  load8f(p + (long long)W * C, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = fmaxf(a[e], b[e]);
  load8f(p + (long long)W * C + C, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = fmaxf(a[e], b[e]);
  store8f(out + (((long long)n * Ho + oy) * Wo + ox) * C + c, a);
}

// its gradient: one thread per INPUT pixel and 8 channels.  The gradient of a window goes to its first maximum in row-major order; a
// row or column that the floor dropped receives 0.  relu != 0: times the ReLU mask a > 0 of the saved input.
__global__ void vgg_pool_bwd_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ gout, bf16_t* __restrict__ gin, int N, int H, int W,
                                    int C, int relu) {
  const int Ho = H / 2, Wo = W / 2, c8 = C / 8;
  const long long total = (long long)N * H * W * c8;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  long long t = idx;
  const int c = (int)(t % c8) * 8; t /= c8;
  const int x = (int)(t % W); t /= W;
  const int y = (int)(t % H);
  const int n = (int)(t / H);
  const int oy = y >> 1, ox = x >> 1;
  float r[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = 0.f;
  if (oy < Ho && ox < Wo) {
    const int me = (y & 1) * 2 + (x & 1);
    const bf16_t* p = a + (((long long)n * H + 2 * oy) * W + 2 * ox) * C + c;
    float w[4][8], go[8];
    load8f(p, w[0]);
    load8f(p + C, w[1]);
    load8f(p + (long long)W * C, w[2]);
    load8f(p + (long long)W * C + C, w[3]);
    load8f(gout + (((long long)n * Ho + oy) * Wo + ox) * C + c, go);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int best = 0;
      float bv = w[0][e];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (w[k][e] > bv) { bv = w[k][e]; best = k; }
      const bool on = best == me && (!relu || bv > 0.f);
      r[e] = on ? go[e] : 0.f;
    }
  }
  store8f(gin + (((long long)n * H + y) * W + x) * C + c, r);
}

// sum rho(f_x - f_y) over one tap: block b folds the elements 8 (b * 256 + t) + 8 * 256 * nblk * j in fp64, then a tree over the block
__global__ __launch_bounds__(256) void vgg_tap_partial_kernel(const bf16_t* __restrict__ fx, const bf16_t* __restrict__ fy, long long n8,
                                                              M2TPixelLoss sd, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < n8; v += (long long)gridDim.x * 256) {
    float a[8], b[8];
    load8f(fx + v * 8, a);
    load8f(fy + v * 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float term;
      (void)m2t_pixel_loss_eval(sd.kind, a[e] - b[e], sd.param, sd.f0, sd.f1, term);
      s += (double)term;
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

struct VggFold { int nblk[5]; double wn[5]; double inv_n[5]; };    // wn = scale * w_k / N_k, inv_n = 1 / N_k

// part [5][256] -> loss_out (+=), per_tap_out[k] = mean_k
__global__ __launch_bounds__(256) void vgg_finish_kernel(const double* __restrict__ part, VggFold f, int accumulate, float* __restrict__ loss_out,
                                                         double* __restrict__ per_tap_out) {
  __shared__ double red[256];
  double total = 0.0;
  for (int k = 0; k < 5; ++k) {
    red[threadIdx.x] = (int)threadIdx.x < f.nblk[k] ? part[k * 256 + threadIdx.x] : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    const double sum = red[0];
    __syncthreads();
    total += sum * f.wn[k];
    if (threadIdx.x == 0 && per_tap_out) per_tap_out[k] = sum * f.inv_n[k];
  }
  if (threadIdx.x == 0) loss_out[0] = (accumulate ? loss_out[0] : 0.f) + (float)total;
}

// the gradient at relu5_1's convolution output: the seed times the ReLU mask
__global__ void vgg_tap_seed_kernel(const bf16_t* __restrict__ fx, const bf16_t* __restrict__ fy, long long n8, M2TPixelLoss sd,
                                    bf16_t* __restrict__ gout) {
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n8) return;
  float a[8], b[8], r[8];
  load8f(fx + v * 8, a);
  load8f(fy + v * 8, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = a[e] > 0.f ? seed_factor(sd, a[e], b[e]) : 0.f;
  store8f(gout + v * 8, r);
}

int grid1(long long n, int bs) { return (int)((n + bs - 1) / bs); }

}  // namespace

int launch_vgg_conv(int epi, const void* in, const void* wpk, void* out, int N, int H, int W, int Cin, int Cout, const float* bias,
                    const void* mask, const void* ytap, const M2TPixelLoss& sd, hipStream_t st) {
  const int tiles_x = ceil_div(W, TP), tiles_y = ceil_div(H, TP);
  const dim3 grid(tiles_x * tiles_y, Cout / NT, N);
  if (epi == 0)
    vgg_conv3x3_kernel<0><<<grid, 256, 0, st>>>((const bf16_t*)in, (const bf16_t*)wpk, (bf16_t*)out, H, W, Cin, Cout, tiles_x, bias, nullptr,
                                                nullptr, sd);
  else
    vgg_conv3x3_kernel<1><<<grid, 256, 0, st>>>((const bf16_t*)in, (const bf16_t*)wpk, (bf16_t*)out, H, W, Cin, Cout, tiles_x, nullptr,
                                                (const bf16_t*)mask, (const bf16_t*)ytap, sd);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_pack(const float* w, void* dst, int Cout, int Cin, int flip, hipStream_t st) {
  vgg_pack_kernel<<<grid1((long long)Cout * Cin * 9, 256), 256, 0, st>>>(w, (bf16_t*)dst, Cout, Cin, flip);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_pack_first(const float* w, float* dst, hipStream_t st) {
  vgg_pack_first_kernel<<<grid1(27 * 64, 256), 256, 0, st>>>(w, dst);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_first_fwd(const float* x, long long img, long long chs, int row, float R, int clamp, const float* w0, const float* bias,
                         void* out, int N, int H, int W, hipStream_t st) {
  vgg_first_fwd_kernel<<<dim3(grid1((long long)H * W, 256), N), 256, 0, st>>>(x, img, chs, row, R, clamp, w0, bias, (bf16_t*)out, H, W);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_first_bwd(const void* g, const float* w0, const float* x, float* gx, long long img, long long chs, int row, float R, int clamp,
                         int N, int H, int W, hipStream_t st) {
  vgg_first_bwd_kernel<<<dim3(grid1((long long)H * W, 256), N), 256, 0, st>>>((const bf16_t*)g, w0, x, gx, img, chs, row, R, clamp, H, W);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_pool_fwd(const void* in, void* out, int N, int H, int W, int C, hipStream_t st) {
  vgg_pool_fwd_kernel<<<grid1((long long)N * (H / 2) * (W / 2) * (C / 8), 256), 256, 0, st>>>((const bf16_t*)in, (bf16_t*)out, N, H, W, C);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_pool_bwd(const void* a, const void* gout, void* gin, int N, int H, int W, int C, int relu, hipStream_t st) {
  vgg_pool_bwd_kernel<<<grid1((long long)N * H * W * (C / 8), 256), 256, 0, st>>>((const bf16_t*)a, (const bf16_t*)gout, (bf16_t*)gin, N, H, W, C,
                                                                                 relu);
  M2T_LAUNCH_CHECK();
  return 0;
}

int vgg_tap_blocks(long long n_elems) {
  const long long b = (n_elems / 8 + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

int launch_vgg_tap_partial(const void* fx, const void* fy, long long n_elems, const M2TPixelLoss& sd, double* part, hipStream_t st) {
  vgg_tap_partial_kernel<<<vgg_tap_blocks(n_elems), 256, 0, st>>>((const bf16_t*)fx, (const bf16_t*)fy, n_elems / 8, sd, part);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_finish(const double* part, const int* nblk, const double* wn, const double* inv_n, int accumulate, float* loss_out,
                      double* per_tap_out, hipStream_t st) {
  VggFold f;
  for (int k = 0; k < 5; ++k) { f.nblk[k] = nblk[k]; f.wn[k] = wn[k]; f.inv_n[k] = inv_n[k]; }
  vgg_finish_kernel<<<1, 256, 0, st>>>(part, f, accumulate, loss_out, per_tap_out);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_vgg_tap_seed(const void* fx, const void* fy, long long n_elems, const M2TPixelLoss& sd, void* gout, hipStream_t st) {
  vgg_tap_seed_kernel<<<grid1(n_elems / 8, 256), 256, 0, st>>>((const bf16_t*)fx, (const bf16_t*)fy, n_elems / 8, sd, (bf16_t*)gout);
  M2T_LAUNCH_CHECK();
  return 0;
}
