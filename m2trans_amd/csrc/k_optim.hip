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

// =======================================================================================
// Parameter groups (include/m2t_groups.h): the flat buffer is cut into at most M2T_MAX_SEGMENTS contiguous segments, each of which
// belongs to one of at most M2T_MAX_GROUPS groups; a group has its own lr / weight decay / pmul and may be frozen.
//
// The segment table is a device blob the caller uploads once (m2t_group_table_pack wrote it on the host):
//   long long hdr[4] = { n_seg, n_groups, n, 0 } ; long long start[n_seg + 1] (start[0] = 0, start[n_seg] = n, strictly ascending) ;
//   unsigned char gid[n_seg]
// Each workgroup stages it in LDS (one memory latency at kernel entry) and every lane finds the segment of its 16-byte vector by a
// binary search there (<= 10 LDS reads, no dependent global load per element); the per-group values travel by value and are staged
// in LDS too (a per-lane index into a by-value array would live in scratch).  A kernel whose header does not match the launch's (n_seg, n_groups, n) returns without touching anything:
// the indices it would compute could not be trusted.
// =======================================================================================
#define GRP_MAX_GROUPS 8
#define GRP_MAX_SEGMENTS 1024
#define GRP_HDR 4
#define GRP_CHUNK_VECTORS 512            // 16-byte vectors per workgroup chunk of the grouped Adam pass (2 per lane)

struct grp_table_lds {
  long long start[GRP_MAX_SEGMENTS + 1];
  unsigned char gid[GRP_MAX_SEGMENTS];
};

// Staging in two halves so that the table's loads, the header's and whatever the kernel loads next (the optimizer record) are all
// in flight together -- ONE memory latency at kernel entry, not one per dependent step: grp_table_regs::load issues the loads
// (n_seg was bounded on the host, so they stay inside a blob of the size the caller was told to allocate), ::store writes LDS and
// says whether the blob's header is the one this launch was told about (uniform).  The caller puts a barrier behind store().
template <int THREADS>
struct grp_table_regs {
  static constexpr int K = (GRP_MAX_SEGMENTS + THREADS) / THREADS;        // entries per lane: ceil((GRP_MAX_SEGMENTS + 1) / THREADS)
  long long sv[K];
  unsigned char gv[K];
  long long h0, h1, h2;
  __device__ __forceinline__ void load(const long long* __restrict__ tab, int n_seg) {
    const long long* st = tab + GRP_HDR;
    const unsigned char* gid = reinterpret_cast<const unsigned char*>(st + n_seg + 1);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = threadIdx.x + k * THREADS;
      sv[k] = i <= n_seg ? st[i] : 0;
      gv[k] = i < n_seg ? gid[i] : 0;
    }
    h0 = tab[0]; h1 = tab[1]; h2 = tab[2];
  }
  __device__ __forceinline__ bool store(int n_seg, int n_groups, long long n, grp_table_lds& t) const {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = threadIdx.x + k * THREADS;
      if (i <= n_seg) t.start[i] = sv[k];
      if (i < n_seg) t.gid[i] = gv[k];
    }
    return h0 == (long long)n_seg && h1 == (long long)n_groups && h2 == n;
  }
};

// the segment that holds element e (0 <= e < n), known to lie in lo .. hi - 1: start[seg] <= e < start[seg + 1]
__device__ __forceinline__ int grp_find(const grp_table_lds& t, int lo, int hi, long long e) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.start[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// the same for an e that is UNIFORM over a full wave of 64 lanes: two rounds of 64 / 16 probes and a ballot each (the bounds ascend,
// so the lanes whose probe is <= e form a prefix) -- two dependent LDS reads instead of up to ten
__device__ __forceinline__ int grp_find_wave(const grp_table_lds& t, int n_seg, long long e) {
  const int lane = threadIdx.x & 63;
  const int i1 = lane * (GRP_MAX_SEGMENTS / 64);                       // probes 16 apart cover 0 .. 1 023; start[0] = 0 <= e
  const unsigned long long b1 = __ballot(i1 < n_seg && t.start[i1] <= e);
  const int coarse = (__popcll(b1) - 1) * (GRP_MAX_SEGMENTS / 64);
  const int i2 = coarse + (lane & (GRP_MAX_SEGMENTS / 64 - 1));
  const unsigned long long b2 = __ballot(lane < GRP_MAX_SEGMENTS / 64 && i2 < n_seg && t.start[i2] <= e);
  return coarse + __popcll(b2) - 1;
}

// ---- masked gradient norm: grad_norm_partial_kernel with the elements of frozen groups left out.  The same grid, the same element ->
// accumulator mapping and the same order; an element left out is an addition of +0.0 to an accumulator that is never -0.0, so the
// partials carry the bits grad_norm_partial_kernel gives for a copy of g whose frozen ranges are +0.0 -- and a frozen element is never
// loaded, so what it holds (NaN, Inf) cannot matter.
__global__ void __launch_bounds__(M2T_GNORM_THREADS) grad_norm_partial_groups_kernel(const float* __restrict__ g, long long n, int head,
                                                                                     float gscale, double* __restrict__ part,
                                                                                     const long long* __restrict__ tab, int n_seg,
                                                                                     int n_groups, unsigned frozen_mask) {
  __shared__ double red[M2T_GNORM_THREADS / 64];
  __shared__ grp_table_lds T;
  grp_table_regs<M2T_GNORM_THREADS> tr;
  tr.load(tab, n_seg);
  const bool ok = tr.store(n_seg, n_groups, n, T);
  __syncthreads();
  double acc = 0.0;
  if (ok) {
    const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n4 = (n - head) / 4;
    for (long long t = tid; t < n4; t += stride) {
      const long long e = head + 4 * t;
      int seg = grp_find(T, 0, n_seg, e);
      if (e + 4 <= T.start[seg + 1]) {             // the four elements share a segment: one 16-byte load, or none
        if ((frozen_mask >> T.gid[seg]) & 1u) continue;
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double x = (double)(gg[i] * gscale);
          acc += x * x;
        }
      } else {                                     // a vector that straddles a boundary: element by element, in the same order
        for (int i = 0; i < 4; ++i) {
          while (e + i >= T.start[seg + 1]) ++seg;
          if ((frozen_mask >> T.gid[seg]) & 1u) continue;
          const double x = (double)(g[e + i] * gscale);
          acc += x * x;
        }
      }
    }
    if (blockIdx.x == 0) {
      if ((int)threadIdx.x < head) {
        const long long e = threadIdx.x;
        if (!((frozen_mask >> T.gid[grp_find(T, 0, n_seg, e)]) & 1u)) {
          const double x = (double)(g[e] * gscale);
          acc += x * x;
        }
      }
      const long long t0 = head + n4 * 4;          // tail: n - t0 in 0..3
      if ((long long)threadIdx.x < n - t0) {
        const long long e = t0 + threadIdx.x;
        if (!((frozen_mask >> T.gid[grp_find(T, 0, n_seg, e)]) & 1u)) {
          const double x = (double)(g[e] * gscale);
          acc += x * x;
        }
      }
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

int launch_grad_norm_groups(const float* g, long long n, float gscale, float max_norm, int skip_nonfinite, int step, float b1, float b2,
                            double* rec, double* part, const void* table, int n_seg, int n_groups, unsigned frozen_mask,
                            hipStream_t st) {
  int head = (int)(((16 - ((uintptr_t)g & 15)) & 15) / 4);
  if (head > n) head = (int)n;
  hipLaunchKernelGGL(grad_norm_partial_groups_kernel, dim3(M2T_GNORM_BLOCKS), dim3(M2T_GNORM_THREADS), 0, st, g, n, head, gscale, part,
                     (const long long*)table, n_seg, n_groups, frozen_mask);
  M2T_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, part, max_norm, skip_nonfinite, step, b1, b2, rec);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---- grouped Adam: adam_ex_one per element with the element's own group's lr / wd / pmul; everything else is shared.  An element
// of a frozen group is neither read nor written.
struct adam_grp_args {
  adam_ex_args base;                     // b1, b2, eps, gscale, ema_d, bc1, bc2_sqrt; coupled / decoupled = the MODE (a group with wd = 0 has neither)
  float lr[GRP_MAX_GROUPS], wd[GRP_MAX_GROUPS], pmul[GRP_MAX_GROUPS];
  unsigned frozen_mask;
  int n_groups, n_seg;
};

__device__ __forceinline__ adam_ex_args grp_args_of(const adam_ex_args& base, const float lr, const float wd, const float pmul) {
  adam_ex_args a = base;
  a.lr = lr; a.wd = wd; a.pmul = pmul;
  a.coupled = base.coupled && wd != 0.f;
  a.decoupled = base.decoupled && wd != 0.f;
  return a;
}

template <bool EMA>
__global__ void __launch_bounds__(256) adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ ema, long long n,
                                                          const adam_grp_args a, const double* __restrict__ rec,
                                                          const long long* __restrict__ tab) {
  __shared__ grp_table_lds T;
  __shared__ float s_lr[GRP_MAX_GROUPS], s_wd[GRP_MAX_GROUPS], s_pmul[GRP_MAX_GROUPS];
  const int n_seg = a.n_seg;
  grp_table_regs<256> tr;
  tr.load(tab, n_seg);                         // (in flight together with the record's loads below)
  float coef = 1.f, bc1 = a.base.bc1, bc2_sqrt = a.base.bc2_sqrt;
  if (rec) {
    if (rec[REC_APPLIED] == 0.0) return;
    coef = (float)rec[REC_CLIP];
    bc1 = (float)rec[REC_BC1];
    bc2_sqrt = (float)rec[REC_BC2_SQRT];
  }
  if (!tr.store(n_seg, a.n_groups, n, T)) return;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < GRP_MAX_GROUPS; ++i) { s_lr[i] = a.lr[i]; s_wd[i] = a.wd[i]; s_pmul[i] = a.pmul[i]; }    // constant indices
  }
  __syncthreads();
  const float d = a.base.ema_d;
  const unsigned frozen_mask = a.frozen_mask;
  const long long nv = (n + 3) / 4;            // the last vector may be partial: it takes the element path
  // A workgroup owns CONTIGUOUS chunks of GRP_CHUNK_VECTORS vectors: the segments a chunk touches are found once per chunk
  // (two wave-wide searches, uniform over the workgroup), a chunk inside one frozen segment costs nothing more, and a lane's own
  // search runs over the chunk's few segments only -- usually one, i.e. no LDS read at all.
  const long long n_chunks = (nv + GRP_CHUNK_VECTORS - 1) / GRP_CHUNK_VECTORS;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
   const long long e_first = c * (4LL * GRP_CHUNK_VECTORS);
   const long long e_last = (e_first + 4LL * GRP_CHUNK_VECTORS < n ? e_first + 4LL * GRP_CHUNK_VECTORS : n) - 1;
   const int seg_lo = grp_find_wave(T, n_seg, e_first);
   const int seg_hi = grp_find_wave(T, n_seg, e_last);
   if (seg_lo == seg_hi && ((frozen_mask >> T.gid[seg_lo]) & 1u)) continue;
#pragma unroll
   for (int k = 0; k < GRP_CHUNK_VECTORS / 256; ++k) {
    const long long t = c * GRP_CHUNK_VECTORS + k * 256 + threadIdx.x;
    if (t >= nv) continue;
    const long long e = 4 * t;
    int seg = grp_find(T, seg_lo, seg_hi + 1, e);
    if (e + 4 <= T.start[seg + 1]) {           // (start[n_seg] = n: a whole vector inside [0, n))
      const int gi = T.gid[seg];
      if ((frozen_mask >> gi) & 1u) continue;
      const adam_ex_args ga = grp_args_of(a.base, s_lr[gi], s_wd[gi], s_pmul[gi]);
      f32x4 pp = reinterpret_cast<f32x4*>(p)[t];
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[t];
      f32x4 mm = reinterpret_cast<f32x4*>(m)[t];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[t];
      f32x4 ee;
      if (EMA) ee = reinterpret_cast<f32x4*>(ema)[t];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pi = pp[i], mi = mm[i], vi = vv[i];
        adam_ex_one(pi, gg[i], mi, vi, ga, coef, bc1, bc2_sqrt);
        pp[i] = pi; mm[i] = mi; vv[i] = vi;
        if (EMA) ee[i] = d * ee[i] + (1.f - d) * pi;
      }
      reinterpret_cast<f32x4*>(p)[t] = pp;
      reinterpret_cast<f32x4*>(m)[t] = mm;
      reinterpret_cast<f32x4*>(v)[t] = vv;
      if (EMA) reinterpret_cast<f32x4*>(ema)[t] = ee;
    } else {                                   // a boundary inside the vector, or the end of the buffer: element by element
      for (int i = 0; i < 4; ++i) {
        const long long j = e + i;
        if (j >= n) break;
        while (j >= T.start[seg + 1]) ++seg;
        const int gi = T.gid[seg];
        if ((frozen_mask >> gi) & 1u) continue;
        const adam_ex_args ga = grp_args_of(a.base, s_lr[gi], s_wd[gi], s_pmul[gi]);
        float pi = p[j], mi = m[j], vi = v[j];
        adam_ex_one(pi, g[j], mi, vi, ga, coef, bc1, bc2_sqrt);
        p[j] = pi; m[j] = mi; v[j] = vi;
        if (EMA) ema[j] = d * ema[j] + (1.f - d) * pi;
      }
    }
   }
  }
}

int launch_adam_groups(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* lr, float b1, float b2,
                       float eps, int step, float gscale, const float* wd, int decoupled, float ema_d, const double* rec,
                       unsigned frozen_mask, int n_groups, const void* table, int n_seg, hipStream_t st) {
  adam_grp_args a;
  a.base.lr = 0.f; a.base.wd = 0.f; a.base.pmul = 1.f;
  a.base.b1 = b1; a.base.b2 = b2; a.base.eps = eps; a.base.gscale = gscale; a.base.ema_d = ema_d;
  a.base.coupled = !decoupled;
  a.base.decoupled = decoupled != 0;
  a.base.bc1 = (float)(1.0 - pow((double)b1, (double)step));
  a.base.bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
  for (int i = 0; i < GRP_MAX_GROUPS; ++i) {
    a.lr[i] = i < n_groups ? lr[i] : 0.f;
    a.wd[i] = i < n_groups ? wd[i] : 0.f;
    a.pmul[i] = (float)(1.0 - (double)a.lr[i] * (double)a.wd[i]);
  }
  a.frozen_mask = frozen_mask; a.n_groups = n_groups; a.n_seg = n_seg;
  // one workgroup per chunk (every workgroup stages the table once: two vectors per lane instead of adam_ex_kernel's one)
  const long long nv = (n + 3) / 4;
  const int grid = (int)std::min<long long>(std::max<long long>((nv + GRP_CHUNK_VECTORS - 1) / GRP_CHUNK_VECTORS, 1), 1 << 20);
  const dim3 block(256);
  if (ema) hipLaunchKernelGGL(adam_groups_kernel<true>, dim3(grid), block, 0, st, p, g, m, v, ema, n, a, rec, (const long long*)table);
  else hipLaunchKernelGGL(adam_groups_kernel<false>, dim3(grid), block, 0, st, p, g, m, v, ema, n, a, rec, (const long long*)table);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---- the C ABI of include/m2t_groups.h --------------------------------------------------
#include "../../include/m2t_groups.h"
#include <string.h>

static inline size_t grp_gid_offset(int n_seg) { return (size_t)(GRP_HDR + n_seg + 1) * sizeof(long long); }

extern "C" size_t m2t_group_table_bytes(int n_seg) {
  if (n_seg < 1 || n_seg > M2T_MAX_SEGMENTS) return 0;
  return grp_gid_offset(n_seg) + (((size_t)n_seg + 7) & ~(size_t)7);
}

extern "C" int m2t_group_table_pack(const long long* starts, const int* group, int n_seg, long long n, int n_groups, void* blob) {
  if (!starts || !group || !blob) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: null argument");
  if (n_seg < 1 || n_seg > M2T_MAX_SEGMENTS) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: n_seg outside 1 .. M2T_MAX_SEGMENTS");
  if (n_groups < 1 || n_groups > M2T_MAX_GROUPS) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: n_groups outside 1 .. M2T_MAX_GROUPS");
  if (n < 1) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: n < 1");
  if (starts[0] != 0) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: the first segment does not start at 0");
  for (int i = 0; i < n_seg; ++i) {
    if (starts[i + 1] <= starts[i]) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: segment starts are not strictly ascending");
    if (group[i] < 0 || group[i] >= n_groups) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: group id outside 0 .. n_groups - 1");
  }
  if (starts[n_seg] != n) return m2t_set_error(M2T_ERR_ARG, "m2t_group_table_pack: the segments do not end at n");
  memset(blob, 0, m2t_group_table_bytes(n_seg));
  long long* q = (long long*)blob;
  q[0] = n_seg; q[1] = n_groups; q[2] = n; q[3] = 0;
  memcpy(q + GRP_HDR, starts, (size_t)(n_seg + 1) * sizeof(long long));
  unsigned char* gid = (unsigned char*)blob + grp_gid_offset(n_seg);
  for (int i = 0; i < n_seg; ++i) gid[i] = (unsigned char)group[i];
  return 0;
}

// frozen flags -> bit mask; -1 for a bad n_groups / null array
static int grp_frozen_mask(const unsigned char* frozen, int n_groups, unsigned* mask) {
  if (!frozen || n_groups < 1 || n_groups > M2T_MAX_GROUPS) return -1;
  unsigned mk = 0;
  for (int i = 0; i < n_groups; ++i) mk |= frozen[i] ? (1u << i) : 0u;
  *mask = mk;
  return 0;
}

extern "C" int m2t_grad_norm_groups(const float* grads, long long n, float grad_scale, float max_norm, int skip_nonfinite, int step,
                                    float beta1, float beta2, double* record, void* workspace, const unsigned char* frozen,
                                    int n_groups, const void* table, int n_seg, void* stream) {
  unsigned mask = 0;
  if (n < 1 || !grads || !record || !workspace || step < 1 || max_norm != max_norm || !table || n_seg < 1 || n_seg > M2T_MAX_SEGMENTS ||
      (long long)n_seg > n || grp_frozen_mask(frozen, n_groups, &mask) != 0 || ((uintptr_t)grads & 3) || ((uintptr_t)table & 7))
    return m2t_set_error(M2T_ERR_ARG, "m2t_grad_norm_groups: bad argument");
  return launch_grad_norm_groups(grads, n, grad_scale, max_norm, skip_nonfinite != 0, step, beta1, beta2, record, (double*)workspace,
                                 table, n_seg, n_groups, mask, (hipStream_t)stream);
}

extern "C" int m2t_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, const float* lr,
                                    float beta1, float beta2, float eps, int step, float grad_scale, float* ema,
                                    const float* weight_decay, int decoupled, float ema_decay, const double* record,
                                    const unsigned char* frozen, int n_groups, const void* table, int n_seg, void* stream) {
  unsigned mask = 0;
  if (n < 1 || !params || !grads || !exp_avg || !exp_avg_sq || step < 1 || !(ema_decay >= 0.f && ema_decay < 1.f) || !lr ||
      !weight_decay || !table || n_seg < 1 || n_seg > M2T_MAX_SEGMENTS || (long long)n_seg > n ||
      grp_frozen_mask(frozen, n_groups, &mask) != 0 || ((uintptr_t)table & 7))
    return m2t_set_error(M2T_ERR_ARG, "m2t_adam_step_groups: bad argument");
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15))
    return m2t_set_error(M2T_ERR_ARG, "m2t_adam_step_groups: the buffers must be 16-byte aligned");
  for (int i = 0; i < n_groups; ++i)
    if (!(weight_decay[i] >= 0.f) || lr[i] != lr[i])
      return m2t_set_error(M2T_ERR_ARG, "m2t_adam_step_groups: a group's weight decay is negative or NaN, or its lr is NaN");
  return launch_adam_groups(params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, step, grad_scale, weight_decay,
                            decoupled, ema_decay, record, mask, n_groups, table, n_seg, (hipStream_t)stream);
}
