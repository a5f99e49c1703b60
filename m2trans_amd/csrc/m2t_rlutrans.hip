// m2t_rlutrans.hip -- util/rlutrans.py TransBlock.forward behind the C ABI.
//
//   x = x + EffAttention(LayerNorm(x))        util/rlutrans.py:85, 47-67
//   x = x + Mlp(LayerNorm(x))                 util/rlutrans.py:86, 21-27
// dim = 64, 8 heads of 8, Mlp hidden = dim / 4 with ReLU; EffAttention = reduce (64 -> 64, no bias), qkv (64 -> 192, no
// bias), softmax attention INSIDE token chunks of length floor(N / 16) (:53-55 -- a 17th, shorter chunk when N is not a
// multiple of 16), proj (64 -> 64 + bias).  The reference never calls this block (dead code): it is built
// from the library's existing LayerNorm and GEMM kernels plus one small attention kernel.
// m2t_transblock_forward is the inference route; m2t_transblock_forward_train runs the same launches on a workspace that keeps every
// intermediate, and m2t_transblock_backward (include/m2t_rlutrans.h; kernels in k_rlutrans_bwd.hip) walks them back.
#include "../../include/m2t.h"
#include "../../include/m2t_rlutrans.h"
#include "m2t_kernels.h"
#include "m2t_rlutrans_layout.h"

namespace {

// one thread per (token, head): scores against the keys of the token's chunk, softmax (max, then sum -- the order of
// torch.softmax), weighted sum of the values.  qkv [M][192] = q | k | v, each [head][8]; out [M][64] = [head][8]
template <typename T>
__global__ void __launch_bounds__(256) transblock_attn_kernel(const T* __restrict__ qkv, T* __restrict__ out, long long M, int N, int L) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= M * TB_HEADS) return;
  const int head = (int)(t & 7);
  const long long tok = t >> 3;
  const long long b = tok / N;
  const int n = (int)(tok - b * N);
  const int j0 = (n / L) * L, j1 = min(N, j0 + L);
  const float scale = 0.35355339059327379f;       // head_dim ** -0.5, head_dim = 8
  float q[TB_HD];
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) q[d] = to_f(qkv[tok * 192 + head * 8 + d]);
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
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < TB_HD; ++d) s += q[d] * to_f(kp[d]);
    const float e = __expf(s * scale - mx);
    sum += e;
#pragma unroll
    for (int d = 0; d < TB_HD; ++d) acc[d] += e * to_f(kp[64 + d]);
  }
  const float inv = 1.0f / sum;
#pragma unroll
  for (int d = 0; d < TB_HD; ++d) out[tok * 64 + head * 8 + d] = from_f<T>(acc[d] * inv);
}

template <typename T> __global__ void __launch_bounds__(256) tb_to_f32_kernel(const T* __restrict__ s, float* __restrict__ d, long long n) {
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) d[t] = to_f(s[t]);
}

struct TbLayout {
  size_t es, wts, X, Hn, R, QKV, AO, X1, H1, total;
  TbLayout(long long M, int dt) {
    es = dt == M2T_F32 ? 4 : 2;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    wts = o; o += al((size_t)TB_NPARAMS * es);
    X = o; o += al((size_t)M * 64 * es);
    Hn = o; o += al((size_t)M * 64 * es);
    R = o; o += al((size_t)M * 64 * es);
    QKV = o; o += al((size_t)M * 192 * es);
    AO = o; o += al((size_t)M * 64 * es);
    X1 = o; o += al((size_t)M * 64 * es);
    H1 = o; o += al((size_t)M * 16 * es);
    total = o;
  }
};

int tb_gemm(int dt, int emode, const void* A, int K, const void* W, void* Y, int N, long long M, const float* bias, const void* aux,
            hipStream_t st) {
  m2t_gemm_args ga{};
  ga.A = A; ga.lda = K; ga.W = W; ga.Y = Y; ga.ldy = N; ga.bias = bias; ga.aux = aux; ga.ldaux = N;
  ga.M = M; ga.N = N; ga.K = K; ga.H = 1; ga.Wd = 1; ga.r = 1; ga.C = 64;
  return launch_gemm_nt(dt, M2T_A_PLAIN, emode, ga, st);
}

#define CKT(call) do { int rc__ = (call); if (rc__) return rc__; } while (0)

// where the forward's launches read and write: the inference workspace shares one buffer between the two LayerNorm outputs and
// lets fc2 overwrite the reduce output; the training workspace keeps all of them
struct TbForwardBuffers { void *wts, *X, *Hn1, *R, *QKV, *AO, *X1, *Hn2, *H1, *Y; size_t es; };

// the forward, launch by launch; both entry points run exactly this, so their y agree bit for bit
int tb_forward_chain(const float* params, const float* x, float* y, long long M, int N, int dt, const TbForwardBuffers& b, hipStream_t st) {
  auto W = [&](long long off) { return (void*)((char*)b.wts + (size_t)off * b.es); };
  // weights and input in the compute element type (biases / LayerNorm affine stay fp32, read from `params`)
  CKT(launch_convert(dt, params, b.wts, TB_NPARAMS, st));
  CKT(launch_convert(dt, x, b.X, M * 64, st));
  CKT(launch_layernorm(dt, b.X, params + OFF_N1W, params + OFF_N1B, b.Hn1, M, 64, st));                       // :85 norm1
  CKT(tb_gemm(dt, M2T_E_PLAIN, b.Hn1, 64, W(OFF_REDUCE), b.R, 64, M, nullptr, nullptr, st));                 // :48 reduce
  CKT(tb_gemm(dt, M2T_E_PLAIN, b.R, 64, W(OFF_QKV), b.QKV, 192, M, nullptr, nullptr, st));                   // :50 qkv
  {
    const int L = N / 16;                                                                                      // :53-55
    const long long nt = M * TB_HEADS;
    if (dt == M2T_F32) hipLaunchKernelGGL(transblock_attn_kernel<float>, dim3((unsigned)ceil_divll(nt, 256)), dim3(256), 0, st, (const float*)b.QKV, (float*)b.AO, M, N, L);
    else hipLaunchKernelGGL(transblock_attn_kernel<bf16_t>, dim3((unsigned)ceil_divll(nt, 256)), dim3(256), 0, st, (const bf16_t*)b.QKV, (bf16_t*)b.AO, M, N, L);
    M2T_LAUNCH_CHECK();
  }
  CKT(tb_gemm(dt, M2T_E_BIAS_RESID, b.AO, 64, W(OFF_PROJ_W), b.X1, 64, M, params + OFF_PROJ_B, b.X, st));    // :66 proj, :85 + x
  CKT(launch_layernorm(dt, b.X1, params + OFF_N2W, params + OFF_N2B, b.Hn2, M, 64, st));                      // :86 norm2
  CKT(tb_gemm(dt, M2T_E_BIAS_RELU, b.Hn2, 64, W(OFF_FC1W), b.H1, TB_HID, M, params + OFF_FC1B, nullptr, st)); // :22-23 fc1 + ReLU
  CKT(tb_gemm(dt, M2T_E_BIAS_RESID, b.H1, TB_HID, W(OFF_FC2W), b.Y, 64, M, params + OFF_FC2B, b.X1, st));    // :25 fc2, :86 + x
  if (dt == M2T_F32) {
    hipError_t e = hipMemcpyAsync(y, b.Y, (size_t)M * 64 * 4, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  } else {
    hipLaunchKernelGGL(tb_to_f32_kernel<bf16_t>, dim3((unsigned)std::min<long long>(ceil_divll(M * 64, 256), 4096)), dim3(256), 0, st, (const bf16_t*)b.Y, y, M * 64);
    M2T_LAUNCH_CHECK();
  }
  return 0;
}

// dW [Nn][K] slabs = G [M][Nn]^T X [M][K] (both in the storage type)
int tb_wgrad(int dt, const void* G, int Nn, const void* X, int K, long long M, float* slabs, int* ns, hipStream_t st) {
  if ((size_t)wgrad_slab_count(M, Nn, K) > tb_max_slabs(M)) return m2t_set_error(M2T_ERR_STATE, "m2t_transblock_backward: slab arena too small");
  m2t_wgrad_args wa{};
  wa.G = G; wa.ldg = Nn; wa.gmode = M2T_A_PLAIN; wa.X = X; wa.ldx = K; wa.xmode = M2T_A_PLAIN; wa.slabs = slabs; wa.bias_slabs = nullptr;
  wa.M = M; wa.N = Nn; wa.K = K; wa.H = 1; wa.Wd = 1; wa.r = 1; wa.C = 64;
  return launch_wgrad_tn(dt, wa, ns, st);
}

// first stage of a bias gradient: part [*nb][Nn] = column sums of blocks of rows of a [M][Nn]
int tb_colsum(int dt, const void* a, int Nn, long long M, float* part, int* nb, hipStream_t st) {
  return launch_colsum(dt, a, Nn, M, Nn, part, (int)tb_max_colsum_blocks(M), nullptr, 0, st, 0, 0, 0, 1, 64, nb);
}

int tb_check(const char* who, bool null_arg, int B, int N, int dtype) {
  if (null_arg) return m2t_set_error_at(M2T_ERR_ARG, who, "null argument");
  if (dtype != M2T_F32 && dtype != M2T_BF16) return m2t_set_error_at(M2T_ERR_ARG, who, "dtype must be M2T_F32 or M2T_BF16");
  if (B < 1 || N < 16) return m2t_set_error_at(M2T_ERR_ARG, who, "needs B >= 1 and N >= 16 (the reference splits the tokens into chunks of N // 16)");
  return 0;
}

}  // namespace

extern "C" size_t m2t_transblock_workspace_bytes(int B, int N, int dtype) {
  if (B < 1 || N < 1) return 0;
  return TbLayout((long long)B * N, dtype).total;
}

extern "C" int m2t_transblock_forward(const float* params, const float* x, float* y, int B, int N, int dtype, void* workspace,
                                      void* stream) {
  if (!params || !x || !y || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_transblock_forward: null argument");
  if (dtype != M2T_F32 && dtype != M2T_BF16) return m2t_set_error(M2T_ERR_ARG, "m2t_transblock_forward: dtype must be M2T_F32 or M2T_BF16");
  if (B < 1 || N < 16) return m2t_set_error(M2T_ERR_ARG, "m2t_transblock_forward: needs B >= 1 and N >= 16 (the reference splits the tokens into chunks of N // 16)");
  const long long M = (long long)B * N;
  const TbLayout lo(M, dtype);
  char* ws = (char*)workspace;
  const TbForwardBuffers b{ws + lo.wts, ws + lo.X, ws + lo.Hn, ws + lo.R, ws + lo.QKV, ws + lo.AO, ws + lo.X1, ws + lo.Hn, ws + lo.H1, ws + lo.R, lo.es};
  return tb_forward_chain(params, x, y, M, N, dtype, b, (hipStream_t)stream);
}

// ---- the training route (include/m2t_rlutrans.h) --------------------------------------------------------------------------------

extern "C" size_t m2t_transblock_train_workspace_bytes(int B, int N, int dtype) {
  if (B < 1 || N < 16 || (dtype != M2T_F32 && dtype != M2T_BF16)) return 0;
  return TbTrainLayout((long long)B * N, dtype == M2T_F32).total;
}

extern "C" size_t m2t_transblock_train_workspace_offset(int B, int N, int dtype, int region) {
  if (B < 1 || N < 16 || (dtype != M2T_F32 && dtype != M2T_BF16)) return (size_t)-1;
  const TbTrainLayout lo((long long)B * N, dtype == M2T_F32);
  switch (region) {
    case TB_R_H1: return lo.H1;
    case TB_R_AO: return lo.AO;
    case TB_R_WTS: return lo.wts;
    case TB_R_X: return lo.X;
    case TB_R_HN1: return lo.Hn1;
    case TB_R_R: return lo.R;
    case TB_R_QKV: return lo.QKV;
    case TB_R_X1: return lo.X1;
    case TB_R_HN2: return lo.Hn2;
    default: return (size_t)-1;
  }
}

extern "C" int m2t_transblock_forward_train(const float* params, const float* x, float* y, int B, int N, int dtype, void* workspace,
                                            void* stream) {
  CKT(tb_check("m2t_transblock_forward_train", !params || !x || !y || !workspace, B, N, dtype));
  hipStream_t st = (hipStream_t)stream;
  const long long M = (long long)B * N;
  const TbTrainLayout lo(M, dtype == M2T_F32);
  char* ws = (char*)workspace;
  const TbForwardBuffers b{ws + lo.wts, ws + lo.X, ws + lo.Hn1, ws + lo.R, ws + lo.QKV, ws + lo.AO, ws + lo.X1, ws + lo.Hn2, ws + lo.H1, ws + lo.Y, lo.es};
  CKT(tb_forward_chain(params, x, y, M, N, dtype, b, st));
  // the transposed weights of the backward's data-gradient GEMMs (Y = A W^T wants W as [out][in] of the GRADIENT product)
  auto WT = [&](long long off) { return (void*)(ws + lo.wts + (size_t)off * lo.es); };
  CKT(launch_transpose_convert(dtype, params + OFF_FC1W, WT(OFF_FC1T), 16, 64, 16, 0, st));
  CKT(launch_transpose_convert(dtype, params + OFF_PROJ_W, WT(OFF_PROJT), 64, 64, 64, 0, st));
  CKT(launch_transpose_convert(dtype, params + OFF_QKV, WT(OFF_QKVT), 192, 64, 192, 0, st));
  CKT(launch_transpose_convert(dtype, params + OFF_REDUCE, WT(OFF_REDUCET), 64, 64, 64, 0, st));
  return 0;
}

extern "C" int m2t_transblock_backward(const float* params, const float* gy, float* gx, float* gparams, int B, int N, int dtype,
                                       void* workspace, void* stream) {
  CKT(tb_check("m2t_transblock_backward", !params || !gy || !workspace, B, N, dtype));
  if (!gx && !gparams) return m2t_set_error(M2T_ERR_ARG, "m2t_transblock_backward: gx and gparams are both null (nothing to compute)");
  hipStream_t st = (hipStream_t)stream;
  const int dt = dtype;
  const bool f32 = dt == M2T_F32, wantp = gparams != nullptr;
  const long long M = (long long)B * N;
  const TbTrainLayout lo(M, f32);
  char* ws = (char*)workspace;
  auto W = [&](long long off) { return (const void*)(ws + lo.wts + (size_t)off * lo.es); };
  const void *X = ws + lo.X, *Hn1 = ws + lo.Hn1, *R = ws + lo.R, *QKV = ws + lo.QKV, *AO = ws + lo.AO, *X1 = ws + lo.X1, *Hn2 = ws + lo.Hn2,
             *H1 = ws + lo.H1;
  void *gH1 = ws + lo.gH1, *gA = ws + lo.gA, *gB = ws + lo.gB, *gQKV = ws + lo.gQKV;
  float* gX1f = (float*)(ws + lo.gX1f);
  float* arena = (float*)(ws + lo.arena);
  // the residual-stream gradient stays fp32 (gy, gX1f, gx); GEMM operands are in the storage type: fp32 mode reads gy / gX1f themselves
  const void* gyT = f32 ? (const void*)gy : (const void*)(ws + lo.gyT);
  void* gX1t = f32 ? (void*)gX1f : (void*)(ws + lo.gX1t);
  int ns_wr = 0, ns_wqkv = 0, ns_wp = 0, ns_w1 = 0, ns_w2 = 0, nb_bp = 0, nb_b1 = 0, nb_b2 = 0, nb_ln1 = 0, nb_ln2 = 0;
  if (!f32) CKT(launch_convert(dt, gy, ws + lo.gyT, M * 64, st));
  // 1. fc2
  CKT(launch_tb_fc2_dgrad_relu(dt, gyT, W(OFF_FC2W), H1, gH1, M, st));
  if (wantp) {
    CKT(tb_wgrad(dt, gyT, 64, H1, 16, M, arena + lo.a_w2, &ns_w2, st));
    CKT(tb_colsum(dt, gyT, 64, M, arena + lo.a_b2, &nb_b2, st));
  }
  // 2. fc1
  CKT(tb_gemm(dt, M2T_E_PLAIN, gH1, 16, W(OFF_FC1T), gA, 64, M, nullptr, nullptr, st));                      // gHn2
  if (wantp) {
    CKT(tb_wgrad(dt, gH1, 16, Hn2, 64, M, arena + lo.a_w1, &ns_w1, st));
    CKT(tb_colsum(dt, gH1, 16, M, arena + lo.a_b1, &nb_b1, st));
    CKT(launch_tb_ln_affine(dt, X1, gA, arena + lo.a_ln2, M, &nb_ln2, st));
  }
  // 3. norm2: gX1 = gy + LNbwd(gHn2)
  CKT(launch_layernorm_bwd(dt, X1, gA, params + OFF_N2W, gy, gX1f, f32 ? nullptr : gX1t, M, 64, st));
  // 4. proj
  CKT(tb_gemm(dt, M2T_E_PLAIN, gX1t, 64, W(OFF_PROJT), gB, 64, M, nullptr, nullptr, st));                    // gAO
  if (wantp) {
    CKT(tb_wgrad(dt, gX1t, 64, AO, 64, M, arena + lo.a_wp, &ns_wp, st));
    CKT(tb_colsum(dt, gX1t, 64, M, arena + lo.a_bp, &nb_bp, st));
  }
  // 5. attention inside the chunks
  CKT(launch_tb_attn_bwd(dt, QKV, AO, gB, gQKV, (float*)(ws + lo.stats), M, N, st));
  // 6. qkv
  CKT(tb_gemm(dt, M2T_E_PLAIN, gQKV, 192, W(OFF_QKVT), gA, 64, M, nullptr, nullptr, st));                    // gR
  if (wantp) CKT(tb_wgrad(dt, gQKV, 192, R, 64, M, arena + lo.a_wqkv, &ns_wqkv, st));
  // 7. reduce
  CKT(tb_gemm(dt, M2T_E_PLAIN, gA, 64, W(OFF_REDUCET), gB, 64, M, nullptr, nullptr, st));                    // gHn1
  if (wantp) {
    CKT(tb_wgrad(dt, gA, 64, Hn1, 64, M, arena + lo.a_wr, &ns_wr, st));
    CKT(launch_tb_ln_affine(dt, X, gB, arena + lo.a_ln1, M, &nb_ln1, st));
  }
  // 8. norm1: gx = gX1 + LNbwd(gHn1)
  if (gx) CKT(launch_layernorm_bwd(dt, X, gB, params + OFF_N1W, gX1f, gx, nullptr, M, 64, st));
  // second stage of every parameter gradient
  if (wantp) {
    tb_reduce_table tab{};
    int nd = 0;
    auto add = [&](size_t src, long long dst, int n, int ns) { tab.d[nd++] = tb_reduce_desc{(long long)src, dst, n, ns}; };
    add(lo.a_wr, OFF_REDUCE, 64 * 64, ns_wr);
    add(lo.a_wqkv, OFF_QKV, 192 * 64, ns_wqkv);
    add(lo.a_wp, OFF_PROJ_W, 64 * 64, ns_wp);
    add(lo.a_bp, OFF_PROJ_B, 64, nb_bp);
    add(lo.a_ln1, OFF_N1W, 128, nb_ln1);               // norm1.weight | norm1.bias are adjacent
    add(lo.a_w1, OFF_FC1W, 16 * 64, ns_w1);
    add(lo.a_b1, OFF_FC1B, 16, nb_b1);
    add(lo.a_w2, OFF_FC2W, 64 * 16, ns_w2);
    add(lo.a_b2, OFF_FC2B, 64, nb_b2);
    add(lo.a_ln2, OFF_N2W, 128, nb_ln2);               // norm2.weight | norm2.bias
    CKT(launch_tb_param_reduce(arena, gparams, tab, nd, st));
  }
  return 0;
}
