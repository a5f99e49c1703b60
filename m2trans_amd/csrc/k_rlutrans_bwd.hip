// k_rlutrans_bwd.hip -- the kernels of the TransBlock backward (include/m2t_rlutrans.h) that the library did not have yet:
// the ReLU-masked fc2 data gradient, the backward of the chunked attention, the LayerNorm affine gradients and the one-launch
// reduction of every parameter-gradient partial.  The GEMMs, the LayerNorm data gradient and the bias column sums are the
// library's own (k_gemm.hip, k_swin_bwd.hip, k_pointwise.hip); the sequence is in m2t_rlutrans.hip.
// No atomics anywhere: every output element has one owner thread, every sum runs in a fixed order.
#include "m2t_kernels.h"
#include "m2t_rlutrans_layout.h"

namespace {

// gH1[m][j] = [H1[m][j] > 0] * sum_c gy[m][c] W2[c][j]          (Mlp.fc2 data gradient through the ReLU, util/rlutrans.py:23-25)
// one thread per (token, hidden unit); W2 [64][16] sits in LDS as fp32; c ascending
template <typename T>
__global__ void __launch_bounds__(256) tb_fc2_dgrad_relu_kernel(const T* __restrict__ gy, const T* __restrict__ w2, const T* __restrict__ h1,
                                                                T* __restrict__ gh1, long long M) {
  __shared__ float W[64 * 16];
  for (int i = threadIdx.x; i < 64 * 16; i += 256) W[i] = to_f(w2[i]);
  __syncthreads();
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= M * TB_HID) return;
  const int j = (int)(t & 15);
  const long long tok = t >> 4;
  float acc = 0.f;
  if (to_f(h1[t]) > 0.f) {
    const T* g = gy + tok * 64;
#pragma unroll 8
    for (int c = 0; c < 64; ++c) acc += to_f(g[c]) * W[c * 16 + j];
  }
  gh1[t] = from_f<T>(acc);
}

// Attention backward, query side.  One thread per (token i, head): the softmax statistics exactly as transblock_attn_kernel
// takes them (maximum, then sum, keys ascending), delta_i = sum_d gAO_i[d] AO_i[d], and
//   gQ_i = scale * sum_j P_ij (gAO_i . v_j - delta_i) k_j,     P_ij = exp(scale q_i . k_j - max_i) / sum_i
// stats [M * 8][3] = (max_i, 1 / sum_i, delta_i) for the key-side kernel.  gqkv [M][192]: the q third is written here.
template <typename T>
__global__ void __launch_bounds__(256) tb_attn_bwd_q_kernel(const T* __restrict__ qkv, const T* __restrict__ ao, const T* __restrict__ gao,
                                                            T* __restrict__ gqkv, float* __restrict__ stats, long long M, int N, int L) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= M * TB_HEADS) return;
  const int head = (int)(t & 7);
  const long long tok = t >> 3;
  const long long b = tok / N;
  const int n = (int)(tok - b * N);
  const int j0 = (n / L) * L, j1 = min(N, j0 + L);
  const float scale = 0.35355339059327379f;       // head_dim ** -0.5, head_dim = 8
  float q[TB_HD], go[TB_HD];
  float delta = 0.f;
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) {
    q[d] = to_f(qkv[tok * 192 + head * 8 + d]);
    go[d] = to_f(gao[tok * 64 + head * 8 + d]);
    delta += go[d] * to_f(ao[tok * 64 + head * 8 + d]);
  }
  float mx = -3.0e38f;
  for (int j = j0; j < j1; ++j) {
    const T* kp = qkv + (b * N + j) * 192 + 64 + head * 8;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < TB_HD; ++d) s += q[d] * to_f(kp[d]);
    mx = fmaxf(mx, s * scale);
  }
  float sum = 0.f, acc[TB_HD];
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) acc[d] = 0.f;
  for (int j = j0; j < j1; ++j) {
    const T* kp = qkv + (b * N + j) * 192 + 64 + head * 8;
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < TB_HD; ++d) {
      s += q[d] * to_f(kp[d]);
      dp += go[d] * to_f(kp[64 + d]);
    }
    const float e = __expf(s * scale - mx);
    sum += e;
    const float w = e * (dp - delta);
#pragma unroll
    for (int d = 0; d < TB_HD; ++d) acc[d] += w * to_f(kp[d]);
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) gqkv[tok * 192 + head * 8 + d] = from_f<T>(acc[d] * inv * scale);
  stats[t * 3 + 0] = mx;
  stats[t * 3 + 1] = inv;
  stats[t * 3 + 2] = delta;
}

// Attention backward, key side.  One thread per (token j, head) gathers over the queries i of its chunk (ascending):
//   gV_j = sum_i P_ij gAO_i,     gK_j = scale * sum_i P_ij (gAO_i . v_j - delta_i) q_i
// with P_ij rebuilt from the statistics the query-side kernel left.  Writes the k and v thirds of gqkv.
template <typename T>
__global__ void __launch_bounds__(256) tb_attn_bwd_kv_kernel(const T* __restrict__ qkv, const T* __restrict__ gao, const float* __restrict__ stats,
                                                             T* __restrict__ gqkv, long long M, int N, int L) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= M * TB_HEADS) return;
  const int head = (int)(t & 7);
  const long long tok = t >> 3;
  const long long b = tok / N;
  const int n = (int)(tok - b * N);
  const int i0 = (n / L) * L, i1 = min(N, i0 + L);
  const float scale = 0.35355339059327379f;
  float k[TB_HD], v[TB_HD], gk[TB_HD], gv[TB_HD];
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) {
    k[d] = to_f(qkv[tok * 192 + 64 + head * 8 + d]);
    v[d] = to_f(qkv[tok * 192 + 128 + head * 8 + d]);
    gk[d] = 0.f;
    gv[d] = 0.f;
  }
  for (int i = i0; i < i1; ++i) {
    const long long ti = b * N + i;
    const T* qp = qkv + ti * 192 + head * 8;
    const T* gp = gao + ti * 64 + head * 8;
    const float* sp = stats + (ti * TB_HEADS + head) * 3;
    float qi[TB_HD], gi[TB_HD];
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int d = 0; d < TB_HD; ++d) {
      qi[d] = to_f(qp[d]);
      gi[d] = to_f(gp[d]);
      s += qi[d] * k[d];
      dp += gi[d] * v[d];
    }
    const float p = __expf(s * scale - sp[0]) * sp[1];
    const float gs = p * (dp - sp[2]);
#pragma unroll
    for (int d = 0; d < TB_HD; ++d) {
      gv[d] += p * gi[d];
      gk[d] += gs * qi[d];
    }
  }
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) {
    gqkv[tok * 192 + 64 + head * 8 + d] = from_f<T>(gk[d] * scale);
    gqkv[tok * 192 + 128 + head * 8 + d] = from_f<T>(gv[d]);
  }
}

// The same two kernels for chunks of at least TB_TILE tokens, with the chunk staged in LDS: a workgroup owns TB_TILE = 32 rows of ONE
// chunk (grid x = (batch, chunk), y = tile of the chunk; thread = (row of the tile, head)) and walks the chunk in stages of TB_KT = 64
// tokens, whose rows all eight heads of all 32 rows share: [64][64] fp32 per staged tensor (converted once on the way in).  The
// sums run over the same tokens in the same order with the same operations as in the kernels above, so both forms give the same bits.
#define TB_TILE 32
#define TB_KT 64

// stage `cnt` rows of 64 columns starting at src (row stride 192 or 64 elements) as fp32
template <typename T>
__device__ __forceinline__ void tb_stage_rows(float (*dst)[64], const T* __restrict__ src, int ld, int cnt) {
  for (int idx = threadIdx.x; idx < cnt * 64; idx += 256) dst[idx >> 6][idx & 63] = to_f(src[(long long)(idx >> 6) * ld + (idx & 63)]);
}

template <typename T>
__global__ void __launch_bounds__(256) tb_attn_bwd_q_lds_kernel(const T* __restrict__ qkv, const T* __restrict__ ao, const T* __restrict__ gao,
                                                                T* __restrict__ gqkv, float* __restrict__ stats, int N, int L, int nchunk) {
  __shared__ float Ks[TB_KT][64], Vs[TB_KT][64];
  const int b = blockIdx.x / nchunk, c = blockIdx.x - b * nchunk;
  const int j0 = c * L, j1 = min(N, j0 + L);
  if (j0 + (int)blockIdx.y * TB_TILE >= j1) return;              // (uniform: a tile past the end of a short last chunk)
  const int head = threadIdx.x & 7;
  const int n = j0 + blockIdx.y * TB_TILE + (threadIdx.x >> 3);
  const bool live = n < j1;                                       // a dead row computes on the chunk's first token and stores nothing
  const long long base = (long long)b * N;
  const long long tok = base + (live ? n : j0);
  const float scale = 0.35355339059327379f;
  float q[TB_HD], go[TB_HD];
  float delta = 0.f;
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) {
    q[d] = to_f(qkv[tok * 192 + head * 8 + d]);
    go[d] = to_f(gao[tok * 64 + head * 8 + d]);
    delta += go[d] * to_f(ao[tok * 64 + head * 8 + d]);
  }
  float mx = -3.0e38f;
  for (int s0 = j0; s0 < j1; s0 += TB_KT) {
    const int cnt = min(TB_KT, j1 - s0);
    __syncthreads();
    tb_stage_rows(Ks, qkv + (base + s0) * 192 + 64, 192, cnt);
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < TB_HD; ++d) s += q[d] * Ks[j][head * 8 + d];
      mx = fmaxf(mx, s * scale);
    }
  }
  float sum = 0.f, acc[TB_HD];
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) acc[d] = 0.f;
  for (int s0 = j0; s0 < j1; s0 += TB_KT) {
    const int cnt = min(TB_KT, j1 - s0);
    __syncthreads();
    tb_stage_rows(Ks, qkv + (base + s0) * 192 + 64, 192, cnt);
    tb_stage_rows(Vs, qkv + (base + s0) * 192 + 128, 192, cnt);
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < TB_HD; ++d) {
        s += q[d] * Ks[j][head * 8 + d];
        dp += go[d] * Vs[j][head * 8 + d];
      }
      const float e = __expf(s * scale - mx);
      sum += e;
      const float w = e * (dp - delta);
#pragma unroll
      for (int d = 0; d < TB_HD; ++d) acc[d] += w * Ks[j][head * 8 + d];
    }
  }
  if (!live) return;
  const float inv = 1.0f / sum;
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) gqkv[tok * 192 + head * 8 + d] = from_f<T>(acc[d] * inv * scale);
  const long long t = tok * TB_HEADS + head;
  stats[t * 3 + 0] = mx;
  stats[t * 3 + 1] = inv;
  stats[t * 3 + 2] = delta;
}

template <typename T>
__global__ void __launch_bounds__(256) tb_attn_bwd_kv_lds_kernel(const T* __restrict__ qkv, const T* __restrict__ gao, const float* __restrict__ stats,
                                                                 T* __restrict__ gqkv, int N, int L, int nchunk) {
  __shared__ float Qs[TB_KT][64], Gs[TB_KT][64], Ss[TB_KT * TB_HEADS * 3];
  const int b = blockIdx.x / nchunk, c = blockIdx.x - b * nchunk;
  const int i0 = c * L, i1 = min(N, i0 + L);
  if (i0 + (int)blockIdx.y * TB_TILE >= i1) return;
  const int head = threadIdx.x & 7;
  const int n = i0 + blockIdx.y * TB_TILE + (threadIdx.x >> 3);
  const bool live = n < i1;
  const long long base = (long long)b * N;
  const long long tok = base + (live ? n : i0);
  const float scale = 0.35355339059327379f;
  float k[TB_HD], v[TB_HD], gk[TB_HD], gv[TB_HD];
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) {
    k[d] = to_f(qkv[tok * 192 + 64 + head * 8 + d]);
    v[d] = to_f(qkv[tok * 192 + 128 + head * 8 + d]);
    gk[d] = 0.f;
    gv[d] = 0.f;
  }
  for (int s0 = i0; s0 < i1; s0 += TB_KT) {
    const int cnt = min(TB_KT, i1 - s0);
    __syncthreads();
    tb_stage_rows(Qs, qkv + (base + s0) * 192, 192, cnt);
    tb_stage_rows(Gs, gao + (base + s0) * 64, 64, cnt);
    for (int idx = threadIdx.x; idx < cnt * TB_HEADS * 3; idx += 256) Ss[idx] = stats[(base + s0) * TB_HEADS * 3 + idx];
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const float* sp = &Ss[(i * TB_HEADS + head) * 3];
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < TB_HD; ++d) {
        s += Qs[i][head * 8 + d] * k[d];
        dp += Gs[i][head * 8 + d] * v[d];
      }
      const float p = __expf(s * scale - sp[0]) * sp[1];
      const float gs = p * (dp - sp[2]);
#pragma unroll
      for (int d = 0; d < TB_HD; ++d) {
        gv[d] += p * Gs[i][head * 8 + d];
        gk[d] += gs * Qs[i][head * 8 + d];
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) {
    gqkv[tok * 192 + 64 + head * 8 + d] = from_f<T>(gk[d] * scale);
    gqkv[tok * 192 + 128 + head * 8 + d] = from_f<T>(gv[d]);
  }
}

// LayerNorm affine gradients over 64 channels, first stage: block b takes rows [b rpb, (b + 1) rpb), wave w of it every fourth row,
// lane = channel; the row statistics are recomputed the way layernorm_kernel takes them (two-pass, fp32).
//   part[b][c] = sum_rows g[m][c] xhat[m][c]        part[b][64 + c] = sum_rows g[m][c]
template <typename T>
__global__ void __launch_bounds__(256) tb_ln_affine_kernel(const T* __restrict__ x, const T* __restrict__ g, float* __restrict__ part,
                                                           long long M, long long rows_per_block, float eps) {
  __shared__ float sh[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long m0 = blockIdx.x * rows_per_block, m1 = min(M, m0 + rows_per_block);
  float sw = 0.f, sb = 0.f;
  for (long long m = m0 + wv; m < m1; m += 4) {
    const float xv = to_f(x[m * 64 + lane]), gv = to_f(g[m * 64 + lane]);
    const float mean = wave_sum(xv) * (1.0f / 64.0f);
    const float d = xv - mean;
    const float rstd = 1.0f / sqrtf(wave_sum(d * d) * (1.0f / 64.0f) + eps);
    sw += gv * (d * rstd);
    sb += gv;
  }
  sh[wv][lane] = sw;
  sh[wv][64 + lane] = sb;
  __syncthreads();
  if (threadIdx.x < 128) {
    const int c = threadIdx.x;
    part[(long long)blockIdx.x * 128 + c] = (sh[0][c] + sh[1][c]) + (sh[2][c] + sh[3][c]);
  }
}

// second stage of every parameter gradient in one launch: out[dst + e] = sum_s arena[src + s n + e], s in a fixed order
// (four interleaved partial sums, then a fixed combine).  grid (element chunks of 256, descriptor).
__global__ void __launch_bounds__(256) tb_param_reduce_kernel(const float* __restrict__ arena, float* __restrict__ out, tb_reduce_table tab) {
  const tb_reduce_desc d = tab.d[blockIdx.y];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= d.n) return;
  const float* p = arena + d.src + e;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int s = 0;
  for (; s + 3 < d.ns; s += 4) {
    a0 += p[(long long)s * d.n];
    a1 += p[(long long)(s + 1) * d.n];
    a2 += p[(long long)(s + 2) * d.n];
    a3 += p[(long long)(s + 3) * d.n];
  }
  for (; s < d.ns; ++s) a0 += p[(long long)s * d.n];
  out[d.dst + e] = (a0 + a1) + (a2 + a3);
}

}  // namespace

int launch_tb_fc2_dgrad_relu(int dt, const void* gy, const void* w2, const void* h1, void* gh1, long long M, hipStream_t st) {
  const dim3 grid((unsigned)ceil_divll(M * TB_HID, 256));
  if (dt == M2T_F32) hipLaunchKernelGGL(tb_fc2_dgrad_relu_kernel<float>, grid, dim3(256), 0, st, (const float*)gy, (const float*)w2, (const float*)h1, (float*)gh1, M);
  else hipLaunchKernelGGL(tb_fc2_dgrad_relu_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)gy, (const bf16_t*)w2, (const bf16_t*)h1, (bf16_t*)gh1, M);
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_tb_attn_bwd(int dt, const void* qkv, const void* ao, const void* gao, void* gqkv, float* stats, long long M, int N, hipStream_t st) {
  const int L = N / 16;                                            // util/rlutrans.py:53-55
  if (L >= TB_TILE) {                                              // a chunk fills at least one 32-row tile: the LDS-staged form
    const int nchunk = ceil_div(N, L);
    const dim3 lgrid((unsigned)((M / N) * nchunk), (unsigned)ceil_div(L, TB_TILE));
    if (dt == M2T_F32) {
      hipLaunchKernelGGL(tb_attn_bwd_q_lds_kernel<float>, lgrid, dim3(256), 0, st, (const float*)qkv, (const float*)ao, (const float*)gao, (float*)gqkv, stats, N, L, nchunk);
      hipLaunchKernelGGL(tb_attn_bwd_kv_lds_kernel<float>, lgrid, dim3(256), 0, st, (const float*)qkv, (const float*)gao, (const float*)stats, (float*)gqkv, N, L, nchunk);
    } else {
      hipLaunchKernelGGL(tb_attn_bwd_q_lds_kernel<bf16_t>, lgrid, dim3(256), 0, st, (const bf16_t*)qkv, (const bf16_t*)ao, (const bf16_t*)gao, (bf16_t*)gqkv, stats, N, L, nchunk);
      hipLaunchKernelGGL(tb_attn_bwd_kv_lds_kernel<bf16_t>, lgrid, dim3(256), 0, st, (const bf16_t*)qkv, (const bf16_t*)gao, (const float*)stats, (bf16_t*)gqkv, N, L, nchunk);
    }
    M2T_LAUNCH_CHECK();
    return 0;
  }
  const dim3 grid((unsigned)ceil_divll(M * TB_HEADS, 256));
  if (dt == M2T_F32) {
    hipLaunchKernelGGL(tb_attn_bwd_q_kernel<float>, grid, dim3(256), 0, st, (const float*)qkv, (const float*)ao, (const float*)gao, (float*)gqkv, stats, M, N, L);
    hipLaunchKernelGGL(tb_attn_bwd_kv_kernel<float>, grid, dim3(256), 0, st, (const float*)qkv, (const float*)gao, (const float*)stats, (float*)gqkv, M, N, L);
  } else {
    hipLaunchKernelGGL(tb_attn_bwd_q_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)qkv, (const bf16_t*)ao, (const bf16_t*)gao, (bf16_t*)gqkv, stats, M, N, L);
    hipLaunchKernelGGL(tb_attn_bwd_kv_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)qkv, (const bf16_t*)gao, (const float*)stats, (bf16_t*)gqkv, M, N, L);
  }
  M2T_LAUNCH_CHECK();
  return 0;
}

int launch_tb_ln_affine(int dt, const void* x, const void* g, float* part, long long M, int* nblk_out, hipStream_t st) {
  int nblk = (int)tb_max_colsum_blocks(M);
  const long long rpb = ceil_divll(M, nblk);
  nblk = (int)ceil_divll(M, rpb);
  if (dt == M2T_F32) hipLaunchKernelGGL(tb_ln_affine_kernel<float>, dim3(nblk), dim3(256), 0, st, (const float*)x, (const float*)g, part, M, rpb, 1e-5f);
  else hipLaunchKernelGGL(tb_ln_affine_kernel<bf16_t>, dim3(nblk), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)g, part, M, rpb, 1e-5f);
  M2T_LAUNCH_CHECK();
  *nblk_out = nblk;
  return 0;
}

int launch_tb_param_reduce(const float* arena, float* out, const tb_reduce_table& tab, int ndesc, hipStream_t st) {
  int nmax = 0;
  for (int i = 0; i < ndesc; ++i) nmax = std::max(nmax, tab.d[i].n);
  hipLaunchKernelGGL(tb_param_reduce_kernel, dim3(ceil_div(nmax, 256), ndesc), dim3(256), 0, st, arena, out, tab);
  M2T_LAUNCH_CHECK();
  return 0;
}
