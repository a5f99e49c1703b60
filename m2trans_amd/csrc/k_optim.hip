// k_optim.hip -- the optimizer end of the training step over the flat fp32 buffers   (train.py:81,210)
//
//   gradient norm (two stages, fp64, fixed summation tree)  ->  a small device-resident OPTIMIZER RECORD
//   adam_ex_kernel: clip coefficient, coupled / decoupled weight decay, Adam, EMA of the weights in ONE pass,
//                   skipped as a whole when the record says the gradient was not finite
//
// restates   torch.nn.utils.clip_grad_norm_(params, max_norm)                      (the coefficient: fp32, as torch)
//            torch.optim.Adam(lr, betas, eps, weight_decay, decoupled_weight_decay).step()
//            ema.mul_(d).add_(p, alpha=1 - d)
// No atomics, no ticket, no host synchronisation: the record is written by plain stores of one thread and read by the
// big kernel through uniform loads.  adam_kernel (k_pointwise.hip) is the path with every option off and is not touched.
#include "m2t_kernels.h"

// ---- the record: M2T_OPTIM_RECORD_DOUBLES doubles (m2t.h documents the layout for callers) ------------------------
enum { REC_NORM = 0, REC_FINITE = 1, REC_CLIP = 2, REC_APPLIED = 3, REC_SKIPPED = 4, REC_BC1 = 5, REC_BC2_SQRT = 6, REC_STEP = 7 };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// =======================================================================================
// stage 1: part[b] = sum over the elements workgroup b owns of (gscale * g)^2, in fp64.
// The grid is M2T_GNORM_BLOCKS x M2T_GNORM_THREADS (16 waves per workgroup: one workgroup per CU keeps enough 16-byte loads in
// flight for a streaming read) whatever the device and whatever n: which elements meet in which accumulator, and in
// which order, is a function of n and of the pointer's 16-byte phase alone -> the same bits on every run and every device.
// head: elements up to g's next 16-byte boundary; block 0 takes them and the (at most 3) tail elements, as grad_accumulate_kernel.
// =======================================================================================
__global__ void __launch_bounds__(M2T_GNORM_THREADS) grad_norm_partial_kernel(const float* __restrict__ g, long long n, int head,
                                                                              float gscale, double* __restrict__ part) {
  __shared__ double red[M2T_GNORM_THREADS / 64];
  const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long n4 = (n - head) / 4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + head);
  double acc = 0.0;
  for (long long t = tid; t < n4; t += stride) {
    const f32x4 gg = g4[t];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double x = (double)(gg[i] * gscale);
      acc += x * x;
    }
  }
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < head) {
      const double x = (double)(g[threadIdx.x] * gscale);
      acc += x * x;
    }
    const long long t0 = head + n4 * 4;          // tail: n - t0 in 0..3
    if ((long long)threadIdx.x < n - t0) {
      const double x = (double)(g[t0 + threadIdx.x] * gscale);
      acc += x * x;
    }
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < M2T_GNORM_THREADS / 64; ++w) s += red[w];       // in wave order
    part[blockIdx.x] = s;
  }
}

// =======================================================================================
// stage 2: one workgroup; the partials are summed IN INDEX ORDER by one thread, which then writes the record.
//   clip_coef as torch.nn.utils.clip_grad_norm_: max_norm / (float(norm) + 1e-6) clamped to 1, in fp32 (NaN stays NaN)
//   applied   0 iff skip_nonfinite and the norm is not finite; skipped += 1 - applied
//   bc1, sqrt(bc2) for the EFFECTIVE step number t = step - skipped, so the big kernel calls no pow
// =======================================================================================
__global__ void __launch_bounds__(256) grad_norm_finish_kernel(const double* __restrict__ part, float max_norm, int skip_nonfinite,
                                                               int step, float b1, float b2, double* __restrict__ rec) {
  __shared__ double sp[M2T_GNORM_BLOCKS];
  for (int i = threadIdx.x; i < M2T_GNORM_BLOCKS; i += blockDim.x) sp[i] = part[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < M2T_GNORM_BLOCKS; ++i) s += sp[i];
  const double norm = sqrt(s);
  const bool finite = isfinite(norm);
  float coef = 1.f;
  if (max_norm > 0.f) {
    coef = max_norm / ((float)norm + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
  }
  const int applied = (skip_nonfinite && !finite) ? 0 : 1;
  const double skipped = rec[REC_SKIPPED] + (double)(1 - applied);
  const double t = (double)step - skipped;
  rec[REC_NORM] = norm;
  rec[REC_FINITE] = finite ? 1.0 : 0.0;
  rec[REC_CLIP] = (double)coef;
  rec[REC_APPLIED] = (double)applied;
  rec[REC_SKIPPED] = skipped;
  rec[REC_BC1] = 1.0 - pow((double)b1, t);
  rec[REC_BC2_SQRT] = sqrt(1.0 - pow((double)b2, t));
  rec[REC_STEP] = t;
}

int launch_grad_norm(const float* g, long long n, float gscale, float max_norm, int skip_nonfinite, int step, float b1, float b2,
                     double* rec, double* part, hipStream_t st) {
  // elements up to g's next 16-byte boundary (pointers are 4-byte aligned), never more than n
  int head = (int)(((16 - ((uintptr_t)g & 15)) & 15) / 4);
  if (head > n) head = (int)n;
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(M2T_GNORM_BLOCKS), dim3(M2T_GNORM_THREADS), 0, st, g, n, head, gscale, part);
  M2T_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, part, max_norm, skip_nonfinite, step, b1, b2, rec);
  M2T_LAUNCH_CHECK();
  return 0;
}

// =======================================================================================
// Adam with the options, one pass over p, g, m, v (+ ema).  The fp32 operations, in this order (-ffp-contract=off):
//   g' = (g gscale) coef ; coupled: g' = g' + wd p ; decoupled: p = p pmul   (pmul = float32(1 - lr wd), from the host)
//   m = b1 m + (1-b1) g' ; v = b2 v + (1-b2) g' g' ; p = p - (lr/bc1) (m / (sqrt(v)/sqrt(bc2) + eps))
//   ema = d ema + (1-d) p
// rec != nullptr: coef, bc1, sqrt(bc2) and the applied flag come from the record (uniform loads); applied == 0 returns before
// anything is read or written.  g is read only.
// =======================================================================================
struct adam_ex_args {
  float lr, b1, b2, eps, gscale, wd, pmul, ema_d, bc1, bc2_sqrt;
  int coupled, decoupled;
};

__device__ __forceinline__ void adam_ex_one(float& p, const float g, float& m, float& v, const adam_ex_args& a, const float coef,
                                            const float bc1, const float bc2_sqrt) {
  float gi = g * a.gscale * coef;
  if (a.coupled) gi = gi + a.wd * p;
  if (a.decoupled) p = p * a.pmul;
  m = a.b1 * m + (1.f - a.b1) * gi;
  v = a.b2 * v + (1.f - a.b2) * gi * gi;
  const float denom = sqrtf(v) / bc2_sqrt + a.eps;
  p = p - (a.lr / bc1) * (m / denom);
}

template <bool EMA>
__global__ void __launch_bounds__(256) adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ ema, long long n,
                                                      const adam_ex_args a, const double* __restrict__ rec) {
  float coef = 1.f, bc1 = a.bc1, bc2_sqrt = a.bc2_sqrt;
  if (rec) {
    if (rec[REC_APPLIED] == 0.0) return;
    coef = (float)rec[REC_CLIP];
    bc1 = (float)rec[REC_BC1];
    bc2_sqrt = (float)rec[REC_BC2_SQRT];
  }
  const float d = a.ema_d;
  const long long n4 = n / 4;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n4; t += (long long)gridDim.x * blockDim.x) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[t];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[t];
    f32x4 mm = reinterpret_cast<f32x4*>(m)[t];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[t];
    f32x4 ee;
    if (EMA) ee = reinterpret_cast<f32x4*>(ema)[t];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float pi = pp[i], mi = mm[i], vi = vv[i];
      adam_ex_one(pi, gg[i], mi, vi, a, coef, bc1, bc2_sqrt);
      pp[i] = pi; mm[i] = mi; vv[i] = vi;
      if (EMA) ee[i] = d * ee[i] + (1.f - d) * pi;
    }
    reinterpret_cast<f32x4*>(p)[t] = pp;
    reinterpret_cast<f32x4*>(m)[t] = mm;
    reinterpret_cast<f32x4*>(v)[t] = vv;
    if (EMA) reinterpret_cast<f32x4*>(ema)[t] = ee;
  }
  // tail (n not multiple of 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = n4 * 4 + threadIdx.x;
    float pi = p[i], mi = m[i], vi = v[i];
    adam_ex_one(pi, g[i], mi, vi, a, coef, bc1, bc2_sqrt);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if (EMA) ema[i] = d * ema[i] + (1.f - d) * pi;
  }
}

// the grid launch_adam gives adam_kernel for the same n (k_pointwise.hip's grid_for: 256 threads, at most 4096 workgroups)
static inline int adam_grid(long long n) {
  long long g = (n / 4 + 1 + 255) / 256;
  return (int)std::min<long long>(std::max<long long>(g, 1), 256 * 16);
}

int launch_adam_ex(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float b1, float b2, float eps,
                   int step, float gscale, float wd, int decoupled, float ema_d, const double* rec, hipStream_t st) {
  adam_ex_args a;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.gscale = gscale; a.wd = wd; a.ema_d = ema_d;
  a.coupled = (wd != 0.f && !decoupled);
  a.decoupled = (wd != 0.f && decoupled);
  a.pmul = (float)(1.0 - (double)lr * (double)wd);
  // without a record the bias correction is the host's, from `step` (the formula of grad_norm_finish_kernel)
  a.bc1 = (float)(1.0 - pow((double)b1, (double)step));
  a.bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
  const dim3 grid(adam_grid(n)), block(256);
  if (ema) hipLaunchKernelGGL(adam_ex_kernel<true>, grid, block, 0, st, p, g, m, v, ema, n, a, rec);
  else hipLaunchKernelGGL(adam_ex_kernel<false>, grid, block, 0, st, p, g, m, v, ema, n, a, rec);
  M2T_LAUNCH_CHECK();
  return 0;
}
