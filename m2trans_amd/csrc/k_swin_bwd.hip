// k_swin_bwd.hip -- data-gradient kernels of the MedCLIP image tower (Swin-T 224), for the opt-in differentiable
// SemanticLoss (include/m2t.h, "SemanticLoss" section).  The tower is frozen: only d(loss)/d(input pixels) is needed, never a
// weight gradient.  The dense layers' data gradients are gemm_nt launches against transposed weights (k_gemm.hip); this file
// holds what sits between them, in backward order:
//   semantic_loss_bwd   d total / d emb of the SR half
//   swin_head_bwd       L2 normalisation, projection^T, mean-pool broadcast (-> gradient of the final LayerNorm output)
//   layernorm_bwd       every LayerNorm (block, merge, embedding, final), with the fp32 residual-stream gradient added
//   swin_attn_bwd       (shifted) window attention, recomputed from the stashed q|k|v
//   swin_merge_scatter  the inverse of swin_merge_gather
//   swin_embed_bwd      patch-projection^T + the patchify adjoint (fp32 throughout) -> d / d crop pixels
//   bicubic_bwd         the exact adjoint of bicubic_kernel as a deterministic gather
//   add_output_grad     scale * g added into the model's backward seed (m2t_api.hip's gpre)
#include "m2t_kernels.h"

// ---------------------------------------------------------------------------------------
// g_emb[i] = sign(a_i - b_i) / n_patches * t_i / |t_i|   (a_i = emb_i . t^, b_i = emb_{B+i} . t^; sign(0) = 0 as in torch.abs)
// one wave per sample
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) semantic_loss_bwd_kernel(const float* __restrict__ emb, const float* __restrict__ text, int B,
                                                                float inv_np, float* __restrict__ g_emb) {
  const int wv = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wv >= B) return;
  const int i = wv;
  float dx = 0.f, dy = 0.f, tt = 0.f;
  for (int c = lane; c < 512; c += 64) {
    const float t = text[(long long)i * 512 + c];
    dx += emb[(long long)i * 512 + c] * t;
    dy += emb[(long long)(B + i) * 512 + c] * t;
    tt += t * t;
  }
  dx = wave_sum(dx); dy = wave_sum(dy); tt = wave_sum(tt);
  const float rn = 1.0f / sqrtf(tt);
  const float d = dx * rn - dy * rn;
  const float sg = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
  const float k = sg * inv_np * rn;
  for (int c = lane; c < 512; c += 64) g_emb[(long long)i * 512 + c] = k * text[(long long)i * 512 + c];
}
int launch_semantic_loss_bwd(const float* emb, const float* text, int B, int n_patches, float* g_emb, hipStream_t st) {
  hipLaunchKernelGGL(semantic_loss_bwd_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, st, emb, text, B, 1.0f / (float)n_patches, g_emb);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------
// head backward, one workgroup per image.  Recomputes pooled / e / |e| exactly as swin_head_kernel from the stashed final
// LayerNorm output hn [49][768], then
//   g_e = (g - emb (emb . g)) / |e|,   g_pooled = P^T g_e,   g_hn[t] = g_pooled / 49 for every token t
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) swin_head_bwd_kernel(const T* __restrict__ hn, const float* __restrict__ proj,
                                                            const float* __restrict__ g_emb, T* __restrict__ g_hn) {
  __shared__ float pooled[768];
  __shared__ float e[512];
  __shared__ float ge[512];
  __shared__ float red[8];
  const int im = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < 768; c += 256) {
    float s = 0.f;
    for (int t = 0; t < 49; ++t) s += to_f(hn[((long long)im * 49 + t) * 768 + c]);
    pooled[c] = s / 49.0f;
  }
  __syncthreads();
  float ss = 0.f;
  for (int o = tid; o < 512; o += 256) {
    const float* w = proj + (long long)o * 768;
    float a = 0.f;
    for (int c = 0; c < 768; ++c) a = fmaf(pooled[c], w[c], a);
    e[o] = a;
    ss += a * a;
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float inv = 1.0f / sqrtf(red[0] + red[1] + red[2] + red[3]);
  float dp = 0.f;
  for (int o = tid; o < 512; o += 256) dp += e[o] * inv * g_emb[(long long)im * 512 + o];
  dp = wave_sum(dp);
  if ((tid & 63) == 0) red[4 + (tid >> 6)] = dp;
  __syncthreads();
  const float egd = red[4] + red[5] + red[6] + red[7];
  for (int o = tid; o < 512; o += 256) ge[o] = (g_emb[(long long)im * 512 + o] - e[o] * inv * egd) * inv;
  __syncthreads();
  for (int c = tid; c < 768; c += 256) {
    float a = 0.f;
    for (int o = 0; o < 512; ++o) a = fmaf(proj[(long long)o * 768 + c], ge[o], a);
    const T v = from_f<T>(a * (1.0f / 49.0f));
    for (int t = 0; t < 49; ++t) g_hn[((long long)im * 49 + t) * 768 + c] = v;
  }
}
int launch_swin_head_bwd(int dt, const void* hn, const float* proj, const float* g_emb, void* g_hn, int nimg, hipStream_t st) {
  if (dt == M2T_F32) hipLaunchKernelGGL(swin_head_bwd_kernel<float>, dim3(nimg), dim3(256), 0, st, (const float*)hn, proj, g_emb, (float*)g_hn);
  else hipLaunchKernelGGL(swin_head_bwd_kernel<bf16_t>, dim3(nimg), dim3(256), 0, st, (const bf16_t*)hn, proj, g_emb, (bf16_t*)g_hn);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------
// LayerNorm data gradient, one wave per row (lane owns channels lane + 64 i, i < NV), statistics recomputed in fp32 the way
// layernorm_kernel computes them (two-pass):
//   dx = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat)) + resid
// x and g in the storage type; resid / out_f fp32 (the residual-stream gradient, may alias); out_t: the storage-type copy that
// the next data-gradient GEMM reads (the rounding to bf16 happens here, in the producer).  Any of resid / out_f / out_t may be null.
// g_f (optional): the incoming gradient in fp32 instead of g (the embedding LayerNorm, whose output is the residual stream).
// ---------------------------------------------------------------------------------------
template <typename T, int NV>
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ gamma,
                                                            const float* resid, float* out_f, T* __restrict__ out_t, long long M, int C,
                                                            float eps, const float* __restrict__ g_f) {
  const int lane = threadIdx.x & 63;
  const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  const float invC = 1.0f / (float)C;
  for (long long row = wave; row < M; row += nw) {
    float xv[NV], gv[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      const bool ok = c < C;
      xv[i] = ok ? to_f(x[row * C + c]) : 0.f;
      gv[i] = ok ? (g_f ? g_f[row * C + c] : to_f(g[row * C + c])) * gamma[c] : 0.f;
      s += xv[i];
    }
    s = wave_sum(s);
    const float mean = s * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const float d = (lane + 64 * i < C) ? xv[i] - mean : 0.f;
      q += d * d;
    }
    q = wave_sum(q);
    const float rstd = 1.0f / sqrtf(q * invC + eps);
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      xv[i] = (lane + 64 * i < C) ? (xv[i] - mean) * rstd : 0.f;
      sg += gv[i];
      sgx += gv[i] * xv[i];
    }
    sg = wave_sum(sg) * invC;
    sgx = wave_sum(sgx) * invC;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < C) {
        float d = rstd * (gv[i] - sg - xv[i] * sgx);
        if (resid) d += resid[row * C + c];
        if (out_f) out_f[row * C + c] = d;
        if (out_t) out_t[row * C + c] = from_f<T>(d);
      }
    }
  }
}
int launch_layernorm_bwd(int dt, const void* x, const void* g, const float* gamma, const float* resid, float* out_f, void* out_t,
                         long long M, int C, hipStream_t st, float eps, const float* g_f) {
  if (C > 1536) return m2t_set_error(-2, "layernorm_bwd: C must be at most 1536");
  const int g_ = (int)std::min<long long>(ceil_divll(M, 4), 4096);
#define LNB_GO(T_, NV_) hipLaunchKernelGGL((layernorm_bwd_kernel<T_, NV_>), dim3(g_), dim3(256), 0, st, (const T_*)x, (const T_*)g, gamma, \
                                           resid, out_f, (T_*)out_t, M, C, eps, g_f)
#define LNB_T(T_)                                                                                                       \
  if (C <= 128) LNB_GO(T_, 2); else if (C <= 192) LNB_GO(T_, 3); else if (C <= 384) LNB_GO(T_, 6);                     \
  else if (C <= 768) LNB_GO(T_, 12); else LNB_GO(T_, 24);
  if (dt == M2T_F32) { LNB_T(float) } else { LNB_T(bf16_t) }
#undef LNB_T
#undef LNB_GO
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------
// (shifted) window attention backward, one workgroup per (window, head), 49 tokens, head dim 32; the cyclic shift and the window
// partition are index math on the loads / stores exactly as in swin_attn_kernel.  Everything is recomputed from the stashed
// q|k|v in fp32 (LDS): S = q k^T / sqrt(32) + table + (-100 across shift regions), P = softmax(S), then
//   dV = P^T dO,  dP = dO V^T,  dS = P o (dP - rowsum(P o dP)),  dQ = dS K / sqrt(32),  dK = dS^T Q / sqrt(32)
// gqkv [tokens][3C] receives dq | dk | dv of this head; every element is written by exactly one thread.  No table gradient.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) swin_attn_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ table, const T* __restrict__ gout,
                                                            T* __restrict__ gqkv, int H, int W, int C, int heads, int shift) {
  __shared__ float Qs[49][33], Ks[49][33], Vs[49][33], Os[49][33];
  __shared__ float Ps[49][50], Ds[49][50];
  __shared__ long long tok[49];
  __shared__ int reg[49];
  const int tid = threadIdx.x;
  const int head = blockIdx.y;
  const int nwx = W / 7, nwy = H / 7;
  const int wi = blockIdx.x;
  const int wx = wi % nwx, wy = (wi / nwx) % nwy, im = wi / (nwx * nwy);
  if (tid < 49) {
    const int py = tid / 7, px = tid - py * 7;
    int y = wy * 7 + py + shift, x = wx * 7 + px + shift;
    if (y >= H) y -= H;
    if (x >= W) x -= W;
    tok[tid] = ((long long)im * H + y) * W + x;
    const int ry = wy * 7 + py, rx = wx * 7 + px;
    reg[tid] = ((ry >= H - 7) + (ry >= H - shift)) * 3 + (rx >= W - 7) + (rx >= W - shift);
  }
  __syncthreads();
  for (int idx = tid; idx < 49 * 32; idx += 256) {
    const int t = idx >> 5, d = idx & 31;
    const T* base = qkv + tok[t] * (3 * C) + head * 32 + d;
    Qs[t][d] = to_f(base[0]);
    Ks[t][d] = to_f(base[C]);
    Vs[t][d] = to_f(base[2 * C]);
    Os[t][d] = to_f(gout[tok[t] * C + head * 32 + d]);
  }
  __syncthreads();
  const float scale = 0.17677669529663687f;   // 32^-0.5
  for (int idx = tid; idx < 49 * 49; idx += 256) {
    const int i = idx / 49, j = idx - i * 49;
    float s = 0.f, dp = 0.f;
#pragma unroll 8
    for (int d = 0; d < 32; ++d) {
      s = fmaf(Qs[i][d], Ks[j][d], s);
      dp = fmaf(Os[i][d], Vs[j][d], dp);
    }
    const int qy = i / 7, qx = i - qy * 7, ky = j / 7, kx = j - ky * 7;
    float v = s * scale + table[((qy - ky + 6) * 13 + (qx - kx + 6)) * heads + head];
    if (shift > 0 && reg[i] != reg[j]) v += -100.0f;
    Ps[i][j] = v;
    Ds[i][j] = dp;
  }
  __syncthreads();
  if (tid < 49) {
    const int i = tid;
    float mx = -3.0e38f;
    for (int j = 0; j < 49; ++j) mx = fmaxf(mx, Ps[i][j]);
    float sum = 0.f;
    for (int j = 0; j < 49; ++j) { const float e = __expf(Ps[i][j] - mx); Ps[i][j] = e; sum += e; }
    const float inv = 1.0f / sum;
    float rs = 0.f;
    for (int j = 0; j < 49; ++j) { const float p = Ps[i][j] * inv; Ps[i][j] = p; rs += p * Ds[i][j]; }
    for (int j = 0; j < 49; ++j) Ds[i][j] = Ps[i][j] * (Ds[i][j] - rs);
  }
  __syncthreads();
  for (int idx = tid; idx < 49 * 32; idx += 256) {
    const int t = idx >> 5, d = idx & 31;
    float dq = 0.f, dk = 0.f, dv = 0.f;
    for (int u = 0; u < 49; ++u) {
      dq = fmaf(Ds[t][u], Ks[u][d], dq);
      dk = fmaf(Ds[u][t], Qs[u][d], dk);
      dv = fmaf(Ps[u][t], Os[u][d], dv);
    }
    T* base = gqkv + tok[t] * (3 * C) + head * 32 + d;
    base[0] = from_f<T>(dq * scale);
    base[C] = from_f<T>(dk * scale);
    base[2 * C] = from_f<T>(dv);
  }
}
int launch_swin_attn_bwd(int dt, const void* qkv, const float* bias_table, const void* gout, void* gqkv, int nimg, int H, int W, int C,
                         int heads, int shift, hipStream_t st) {
  if (H % 7 || W % 7 || C != heads * 32) return m2t_set_error(-2, "swin_attn_bwd: grid must be a multiple of 7 and head_dim 32");
  dim3 grid(nimg * (H / 7) * (W / 7), heads);
  if (dt == M2T_F32)
    hipLaunchKernelGGL(swin_attn_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)qkv, bias_table, (const float*)gout, (float*)gqkv, H, W,
                       C, heads, shift);
  else
    hipLaunchKernelGGL(swin_attn_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)qkv, bias_table, (const bf16_t*)gout, (bf16_t*)gqkv,
                       H, W, C, heads, shift);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------
// patch-merging scatter (adjoint of swin_merge_gather): gy [n][H/2][W/2][4C] fp32 -> gx [n][H][W][C] as fp32 (the residual-stream
// gradient) and as the storage type (the next GEMM operand).  A permutation: every element written once.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) swin_merge_scatter_kernel(const float* __restrict__ gy, float* __restrict__ gx, T* __restrict__ gxt,
                                                                 int n, int H, int W, int C) {
  const long long total = (long long)n * H * W * C;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(t % C);
    long long r = t / C;
    const int x = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int im = (int)(r / H);
    const int part = (y & 1) | ((x & 1) << 1);
    const float v = gy[(((long long)im * (H / 2) + (y >> 1)) * (W / 2) + (x >> 1)) * (4 * C) + part * C + c];
    gx[t] = v;
    gxt[t] = from_f<T>(v);
  }
}
int launch_swin_merge_scatter(int dt, const float* gy, float* gx, void* gxt, int nimg, int H, int W, int C, hipStream_t st) {
  const long long total = (long long)nimg * H * W * C;
  const int g = (int)std::min<long long>(ceil_divll(total, 256), 4096);
  if (dt == M2T_F32) hipLaunchKernelGGL(swin_merge_scatter_kernel<float>, dim3(g), dim3(256), 0, st, gy, gx, (float*)gxt, nimg, H, W, C);
  else hipLaunchKernelGGL(swin_merge_scatter_kernel<bf16_t>, dim3(g), dim3(256), 0, st, gy, gx, (bf16_t*)gxt, nimg, H, W, C);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------
// patch projection^T + patchify adjoint, fp32: g_crop[im][c][4 ph + ky][4 pw + kx] = sum_o ge[(im, ph, pw)][o] * Wpe[o][c 16 + ky 4 + kx]
// (non-overlapping 4x4 / 4 patches: each output pixel is written once).  Wpe (96 x 48 fp32) lives in LDS.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) swin_embed_bwd_kernel(const float* __restrict__ ge, const float* __restrict__ wpe, float* __restrict__ gc,
                                                             int n) {
  __shared__ float Wl[96 * 48];
  for (int i = threadIdx.x; i < 96 * 48; i += 256) Wl[i] = wpe[i];
  __syncthreads();
  const long long total = (long long)n * 3 * 224 * 224;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t % 224);
    const int y = (int)((t / 224) % 224);
    const int c = (int)((t / (224 * 224)) % 3);
    const long long im = t / (3 * 224 * 224);
    const int k = c * 16 + (y & 3) * 4 + (x & 3);
    const float* g = ge + ((im * 56 + (y >> 2)) * 56 + (x >> 2)) * 96;
    float a = 0.f;
#pragma unroll 8
    for (int o = 0; o < 96; ++o) a = fmaf(g[o], Wl[o * 48 + k], a);
    gc[t] = a;
  }
}
int launch_swin_embed_bwd(const float* ge, const float* wpe, float* g_crops, int nimg, hipStream_t st) {
  const long long total = (long long)nimg * 3 * 224 * 224;
  const int g = (int)std::min<long long>(ceil_divll(total, 256), 2048);
  hipLaunchKernelGGL(swin_embed_bwd_kernel, dim3(g), dim3(256), 0, st, ge, wpe, g_crops, nimg);
  M2T_LAUNCH_CHECK();
  return 0;
}

// fp32 [N][K] -> storage-type transpose: dst[k * ldd + col0 + n] = src[n * K + k]  (weights of the data-gradient GEMMs)
template <typename T>
__global__ void __launch_bounds__(256) transpose_convert_kernel(const float* __restrict__ src, T* __restrict__ dst, int N, int K, int ldd, int col0) {
  const long long total = (long long)N * K;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int nn = (int)(t % N);
    const long long k = t / N;
    dst[k * ldd + col0 + nn] = from_f<T>(src[(long long)nn * K + k]);
  }
}
int launch_transpose_convert(int dt, const float* src, void* dst, int N, int K, int ldd, int col0, hipStream_t st) {
  const int g = (int)std::min<long long>(ceil_divll((long long)N * K, 256), 4096);
  if (dt == M2T_F32) hipLaunchKernelGGL(transpose_convert_kernel<float>, dim3(g), dim3(256), 0, st, src, (float*)dst, N, K, ldd, col0);
  else hipLaunchKernelGGL(transpose_convert_kernel<bf16_t>, dim3(g), dim3(256), 0, st, src, (bf16_t*)dst, N, K, ldd, col0);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------
// bicubic backward (align_corners=True, A = -0.75): the exact adjoint of bicubic_kernel as a GATHER (no atomics, deterministic).
// Source pixel (y, x) collects  sum_{oy, ox} Wy(oy, y) Wx(ox, x) g_dst[oy][ox],  W(o, s) = sum of the tap weights of output o
// whose clamped tap index is s.  Only outputs whose base index floor(s * o) lies in [s - 2, s + 1] can reach s; the candidate
// output range is bounded from that and every candidate is checked with the forward's own index arithmetic.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float cubic1b(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2b(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
__device__ __forceinline__ float bicubic_tap_weight(int o, int s, float scl, int nin) {
  const float A = -0.75f;
  const float f = scl * o;
  const int i0 = (int)floorf(f);
  const float t = f - i0;
  const float w[4] = {cubic2b(t + 1.f, A), cubic1b(t, A), cubic1b(1.f - t, A), cubic2b(2.f - t, A)};
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a)
    if (min(max(i0 - 1 + a, 0), nin - 1) == s) acc += w[a];
  return acc;
}
__device__ __forceinline__ void bicubic_out_range(int s, float scl, int nout, int& lo, int& hi) {
  if (scl <= 0.f) { lo = 0; hi = nout - 1; return; }
  lo = max(0, (int)floorf((float)(s - 2) / scl) - 2);
  hi = min(nout - 1, (int)ceilf((float)(s + 2) / scl) + 2);
}
__global__ void __launch_bounds__(256) bicubic_bwd_kernel(const float* __restrict__ gdst, float* __restrict__ gsrc, int NC, int Hin, int Win,
                                                          int Hout, int Wout) {
  const float sy = (Hout > 1) ? (float)(Hin - 1) / (float)(Hout - 1) : 0.f;
  const float sx = (Wout > 1) ? (float)(Win - 1) / (float)(Wout - 1) : 0.f;
  const long long total = (long long)NC * Hin * Win;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t % Win), y = (int)((t / Win) % Hin);
    const long long nc = t / ((long long)Win * Hin);
    int oy0, oy1, ox0, ox1;
    bicubic_out_range(y, sy, Hout, oy0, oy1);
    bicubic_out_range(x, sx, Wout, ox0, ox1);
    const float* gp = gdst + nc * Hout * Wout;
    float acc = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy) {
      const float wy = bicubic_tap_weight(oy, y, sy, Hin);
      if (wy == 0.f) continue;
      float row = 0.f;
      for (int ox = ox0; ox <= ox1; ++ox) {
        const float wx = bicubic_tap_weight(ox, x, sx, Win);
        if (wx != 0.f) row = fmaf(wx, gp[(long long)oy * Wout + ox], row);
      }
      acc = fmaf(wy, row, acc);
    }
    gsrc[t] = acc;
  }
}
int launch_bicubic_resize_bwd(const float* gdst, float* gsrc, int NC, int Hin, int Win, int Hout, int Wout, hipStream_t st) {
  const long long total = (long long)NC * Hin * Win;
  hipLaunchKernelGGL(bicubic_bwd_kernel, dim3((unsigned)std::min<long long>(ceil_divll(total, 256), 4096)), dim3(256), 0, st, gdst, gsrc, NC, Hin,
                     Win, Hout, Wout);
  M2T_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------
// gpre[b][c][y][x] += scale * g[b][c][y - y0_b][x - x0_b] inside sample b's [gh, gw] block, where the clamp passes the gradient
// (0 <= pre <= R), over the padded [B][3][Hp][Wp] layout of the seed.  Each seed element is touched by one thread.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) add_output_grad_kernel(const float* __restrict__ pre, const float* __restrict__ g, float* __restrict__ gpre,
                                                              int B, int Hp, int Wp, int gh, int gw, M2TCropOrigins org, float scale, float R) {
  const long long total = (long long)B * 3 * gh * gw;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t % gw);
    const int y = (int)((t / gw) % gh);
    const long long bc = t / ((long long)gw * gh);
    const int b = (int)(bc / 3);
    const long long o = (bc * Hp + y + org.y0[b]) * Wp + x + org.x0[b];
    const float v = pre[o];
    if (v >= 0.f && v <= R) gpre[o] += scale * g[t];
  }
}
int launch_add_output_grad(const float* pre, const float* g, float* gpre, int B, int Hp, int Wp, int gh, int gw, const M2TCropOrigins& org,
                           float scale, float R, hipStream_t st) {
  const long long total = (long long)B * 3 * gh * gw;
  hipLaunchKernelGGL(add_output_grad_kernel, dim3((unsigned)std::min<long long>(ceil_divll(total, 256), 4096)), dim3(256), 0, st, pre, g, gpre, B,
                     Hp, Wp, gh, gw, org, scale, R);
  M2T_LAUNCH_CHECK();
  return 0;
}
