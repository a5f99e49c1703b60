// m2t_text.hip -- the MedCLIP TEXT tower behind SemanticLoss (losses.py:22-25,64-65,74): BERT-base
// (emilyalsentzer/Bio_ClinicalBERT geometry: 12 layers, 768 hidden, 12 heads, 3072 intermediate, vocab 28 996, 512
// positions, 2 token types, LayerNorm eps 1e-12, erf GELU) -> mean over the tokens of hidden states 1, 2 and -1 ->
// Linear(768, 512, bias = False) -> L2 normalisation (encode_text of the un-vendored `medclip` package, restated from its
// published source; PARITY UNPINNED: neither the package nor its checkpoint is in the reference tree -- the oracle
// (oracle/text_oracle.py) is checked against transformers.BertModel with random weights).
// Forward only and off the training step's critical path: the reference evaluates it under torch.no_grad() once per
// sample (losses.py:63-65), and because it passes token_type_ids in the input_ids slot (losses.py:65) the result
// depends only on the caption's token COUNT -- m2trans_amd/losses.py caches one embedding per count.
// Built from the library's GEMM (bias / bias + GELU / bias + residual epilogues) and LayerNorm launchers plus three
// small kernels here (embedding + LayerNorm, masked multi-head attention for short sequences, pooling + projection); the fp32
// handle forms q | k | v in a fourth, with fp64 accumulation.
#include "m2t_kernels.h"
#include "m2t_tower.h"
#include "../../include/m2t.h"
#include "../../include/m2t_text.h"

namespace {
constexpr int TX_H = 768, TX_HEADS = 12, TX_DH = 64, TX_FF = 3072, TX_LAYERS = 12, TX_VOCAB = 28996, TX_POS = 512, TX_TYPES = 2;

// embeddings(input_ids, position 0..len-1, token type 0) + LayerNorm(eps 1e-12): one wave per token row
template <typename T>
__global__ void __launch_bounds__(256) text_embed_kernel(const int* __restrict__ ids, const float* __restrict__ word,
                                                         const float* __restrict__ pos, const float* __restrict__ type,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         T* __restrict__ out, int nrows, int len) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nrows) return;
  const int id = min(max(ids[row], 0), TX_VOCAB - 1), t = row % len;
  float v[12];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const int c = lane + 64 * j;
    v[j] = word[(long long)id * TX_H + c] + type[c] + pos[(long long)t * TX_H + c];      // HF order: inputs + token types, + positions
    s += v[j];
  }
  s = wave_sum(s);
  const float mean = s * (1.0f / TX_H);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 12; ++j) { const float d = v[j] - mean; q += d * d; }
  q = wave_sum(q);
  const float rstd = 1.0f / sqrtf(q * (1.0f / TX_H) + 1e-12f);
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const int c = lane + 64 * j;
    out[(long long)row * TX_H + c] = from_f<T>((v[j] - mean) * rstd * gamma[c] + beta[c]);
  }
}

// fp32 handle only: QKV [M][N] = X [M][K] . W [N][K]^T + bias with fp64 ACCUMULATION (a product of two fp32 values is exact in
// fp64) and one rounding, at the store.  The scores are the one place of the tower where an ABSOLUTE error becomes a relative one
// (softmax), so the error of q and k is multiplied by |score|: with scores of +-300 the 6e-7 of an fp32-accumulating GEMM over
// K = 768 came out of the layer as 2e-5 to 3e-5 (tests/test_gpu_text_stages.py, layer 1 of `max`, `edge64`, `allmasked`); the parity
// mode pays an fp64 multiply-add here instead.  64 x 64 outputs per workgroup, 4 x 4 per thread, 16-deep stages.  N % 64 == 0, K % 16 == 0.
__global__ void __launch_bounds__(256) text_qkv_f64acc_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                              const float* __restrict__ bias, float* __restrict__ Y, int M, int N, int K) {
  __shared__ float As[16][65], Ws[16][65];      // [k][row]
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = threadIdx.x + 256 * it, r = idx >> 4, c = idx & 15;
      As[c][r] = (m0 + r < M) ? A[(long long)(m0 + r) * K + k0 + c] : 0.f;
      Ws[c][r] = W[(long long)(n0 + r) * K + k0 + c];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      double a[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = (double)As[kk][ty + 16 * i]; w[i] = (double)Ws[kk][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], w[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 16 * i;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + tx + 16 * j;
      Y[(long long)m * N + n] = (float)(acc[i][j] + (double)bias[n]);
    }
  }
}

// BertSelfAttention for short sequences (len <= 128): one workgroup per (sequence, head), one wave per query row.
// qkv [rows][3 * 768] (q | k | v); scores = q . k / 8 + (mask ? 0 : -inf); softmax; out [rows][768]
// A key is attended iff mask != 0.  A sequence with NO attended key gets uniform weights 1 / len over its len keys: the additive
// finfo.min mask of transformers (and oracle/text_oracle.py) absorbs every score there, so its softmax is uniform.
template <typename T>
__global__ void __launch_bounds__(256) text_attn_kernel(const T* __restrict__ qkv, const int* __restrict__ mask, T* __restrict__ out, int len) {
  __shared__ float Ks[128][TX_DH + 1], Vs[128][TX_DH + 1];
  __shared__ float Ps[4][128];
  const int seq = blockIdx.x / TX_HEADS, head = blockIdx.x % TX_HEADS;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long r0 = (long long)seq * len;
  for (int i = threadIdx.x; i < len * TX_DH; i += 256) {
    const int t = i / TX_DH, d = i % TX_DH;
    Ks[t][d] = to_f(qkv[(r0 + t) * (3 * TX_H) + TX_H + head * TX_DH + d]);
    Vs[t][d] = to_f(qkv[(r0 + t) * (3 * TX_H) + 2 * TX_H + head * TX_DH + d]);
  }
  __syncthreads();
  for (int qi = wv; qi < len; qi += 4) {
    const float qd = to_f(qkv[(r0 + qi) * (3 * TX_H) + head * TX_DH + lane]);      // lane = head dimension
    float sc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int key = lane + 64 * h;
      float a = 0.f;
      for (int d = 0; d < TX_DH; ++d) a += __shfl(qd, d) * ((key < len) ? Ks[key][d] : 0.f);
      sc[h] = (key < len && mask[r0 + key] != 0) ? a * 0.125f : -3.0e38f;
    }
    float mx = fmaxf(sc[0], sc[1]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float e0 = (sc[0] > -1.0e38f) ? __expf(sc[0] - mx) : 0.f, e1 = (sc[1] > -1.0e38f) ? __expf(sc[1] - mx) : 0.f;
    const float sum = wave_sum(e0 + e1);
    const bool none = !(sum > 0.f);                        // no attended key: the uniform rule above
    const float inv = none ? 0.f : 1.0f / sum, uni = 1.0f / (float)len;
    Ps[wv][lane] = none ? (lane < len ? uni : 0.f) : e0 * inv;
    Ps[wv][lane + 64] = none ? (lane + 64 < len ? uni : 0.f) : e1 * inv;
    __builtin_amdgcn_wave_barrier();
    float o = 0.f;
    for (int key = 0; key < len; ++key) o += Ps[wv][key] * Vs[key][lane];
    out[(r0 + qi) * TX_H + head * TX_DH + lane] = from_f<T>(o);
    __builtin_amdgcn_wave_barrier();
  }
}

// pooled[seq][c] (+)= mean over the tokens of H[seq][t][c]  (UNMASKED mean, as the package takes it: `.mean(2)`)
template <typename T>
__global__ void __launch_bounds__(256) text_pool_kernel(const T* __restrict__ Hs, float* __restrict__ pooled, int len, int accumulate) {
  const int seq = blockIdx.x;
  for (int c = threadIdx.x; c < TX_H; c += 256) {
    float a = 0.f;
    for (int t = 0; t < len; ++t) a += to_f(Hs[((long long)seq * len + t) * TX_H + c]);
    a /= (float)len;
    pooled[(long long)seq * TX_H + c] = accumulate ? pooled[(long long)seq * TX_H + c] + a : a;
  }
}
// emb[seq] = normalise(proj [512][768] . (pooled[seq] / 3))
__global__ void __launch_bounds__(512) text_head_kernel(const float* __restrict__ pooled, const float* __restrict__ proj, float* __restrict__ emb) {
  __shared__ float xs[TX_H];
  __shared__ float part[8];
  const int seq = blockIdx.x, o = threadIdx.x;
  for (int c = threadIdx.x; c < TX_H; c += 512) xs[c] = pooled[(long long)seq * TX_H + c] * (1.0f / 3.0f);
  __syncthreads();
  float a = 0.f;
  for (int c = 0; c < TX_H; ++c) a += proj[(long long)o * TX_H + c] * xs[c];
  const float ss = wave_sum(a * a);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) tot += part[i];
  emb[(long long)seq * 512 + o] = a / sqrtf(tot);
}
}  // namespace

// ---- names resolved once, at m2t_text_create: parameter offsets in floats, workspace offsets in bytes ----
struct text_layer {
  m2t_tower_layer L;
  long long ln1_w, ln1_b, ln2_w, ln2_b;      // attention.output.LayerNorm, output.LayerNorm
};
struct text_handles {
  text_layer lyr[TX_LAYERS];
  long long word, pos, type, eln_w, eln_b, head_w;
  size_t packed, fbias, ids, mask, X, XM, Y, QKV, AO, MH, pooled;
};

struct m2t_text {
  int max_seqs, max_len, dt;
  m2t_layout lay;                            // names -> offsets: read by m2t_text_query / m2t_text_param_name only
  text_handles hd;
  const float* weights = nullptr;
};

extern "C" int m2t_text_create(m2t_text** out, int max_seqs, int max_len, int dtype) {
  if (!out || max_seqs < 1 || max_len < 1 || max_len > 128 || (dtype != M2T_F32 && dtype != M2T_BF16))
    return m2t_set_error(M2T_ERR_ARG, "m2t_text_create: bad argument (1 <= max_len <= 128)");
  m2t_text* p = new m2t_text();
  p->max_seqs = max_seqs; p->max_len = max_len; p->dt = dtype; p->lay.esz = (dtype == M2T_F32) ? 4 : 2;
  m2t_layout& lay = p->lay;
  text_handles& hd = p->hd;
  // parameter inventory: HF BertModel checkpoint names (transformers 4.24; `pooler.*` is not used by encode_text and is
  // not part of the buffer) + the MedCLIP text projection
  hd.word = lay.add_param("embeddings.word_embeddings.weight", (long long)TX_VOCAB * TX_H);
  hd.pos = lay.add_param("embeddings.position_embeddings.weight", (long long)TX_POS * TX_H);
  hd.type = lay.add_param("embeddings.token_type_embeddings.weight", (long long)TX_TYPES * TX_H);
  hd.eln_w = lay.add_param("embeddings.LayerNorm.weight", TX_H);
  hd.eln_b = lay.add_param("embeddings.LayerNorm.bias", TX_H);
  for (int l = 0; l < TX_LAYERS; ++l) {
    const std::string b = "encoder.layer." + std::to_string(l) + ".";
    text_layer& ly = hd.lyr[l];
    ly.L.C = TX_H; ly.L.FF = TX_FF;
    tower_add_qkv(lay, b, ly.L);
    tower_add_o(lay, b, ly.L);
    ly.ln1_w = lay.add_param(b + "attention.output.LayerNorm.weight", TX_H);
    ly.ln1_b = lay.add_param(b + "attention.output.LayerNorm.bias", TX_H);
    tower_add_mlp(lay, b, ly.L);
    ly.ln2_w = lay.add_param(b + "output.LayerNorm.weight", TX_H);
    ly.ln2_b = lay.add_param(b + "output.LayerNorm.bias", TX_H);
    tower_add_packs(lay, b, ly.L);
  }
  hd.head_w = lay.add_param("projection_head.weight", 512LL * TX_H);
  const size_t rows = (size_t)max_seqs * max_len, es = lay.esz;
  hd.packed = lay.ws.add("packed", (size_t)lay.npacked, es);
  hd.fbias = lay.ws.add("fbias", (size_t)lay.nfb, 4);
  hd.ids = lay.ws.add("ids", rows, 4);
  hd.mask = lay.ws.add("mask", rows, 4);
  hd.X = lay.ws.add("X", rows * TX_H, es);
  hd.XM = lay.ws.add("XM", rows * TX_H, es);      // the attention-block LayerNorm of a layer (kept apart from X so every stage input survives)
  hd.Y = lay.ws.add("Y", rows * TX_H, es);
  hd.QKV = lay.ws.add("QKV", rows * 3 * TX_H, es);
  hd.AO = lay.ws.add("AO", rows * TX_H, es);
  hd.MH = lay.ws.add("MH", rows * TX_FF, es);
  hd.pooled = lay.ws.add("pooled", (size_t)max_seqs * TX_H, 4);
  lay.ws.seal();
  *out = p;
  return 0;
}
extern "C" void m2t_text_destroy(m2t_text* p) { delete p; }
extern "C" long long m2t_text_query(const m2t_text* p, const char* key) {
  if (!p || !key) return -1;
  const std::string k(key);
  if (k == "max_seqs") return p->max_seqs;
  if (k == "max_len") return p->max_len;
  return p->lay.query(k, m2t_layout::Q_WS | m2t_layout::Q_WSN);      // (no packed: keys on this handle)
}
extern "C" const char* m2t_text_param_name(const m2t_text* p, int i) {
  return p ? p->lay.param_name(i) : nullptr;
}

// once per weight set: the frozen fp32 weights -> element type T, q | k | v fused into one [2304][768] matrix per layer
extern "C" int m2t_text_load_weights(m2t_text* p, const float* weights, void* workspace, void* stream) {
  if (!p || !weights || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_text_load_weights: null");
  p->weights = weights;
  for (int l = 0; l < TX_LAYERS; ++l)
    CK(tower_pack_layer(p->dt, p->lay.esz, p->hd.lyr[l].L, weights, (char*)workspace + p->hd.packed, (float*)((char*)workspace + p->hd.fbias),
                        (hipStream_t)stream));
  return 0;
}

// medmodel.encode_text(input_ids, attention_mask) (losses.py:65,74): ids_host / mask_host int[n][len] in HOST memory
// (the reference passes `token_type_ids` as input_ids: the caller reproduces that by passing those values here)
// -> emb [n][512] fp32 on the device, unit L2 norm
// hidden_out (nullable): [13][n][len][768] of T on the device <- X after the embedding and after each layer (HF hidden_states)
extern "C" int m2t_text_encode_ex(m2t_text* p, const int* ids_host, const int* mask_host, int n, int len, float* emb, void* workspace,
                                  void* stream, void* hidden_out) {
  if (!p || !ids_host || !mask_host || !emb || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_text_encode: null argument");
  if (!p->weights) return m2t_set_error(M2T_ERR_STATE, "m2t_text_encode: call m2t_text_load_weights first");
  if (n < 1 || n > p->max_seqs || len < 1 || len > p->max_len) return m2t_set_error(M2T_ERR_ARG, "m2t_text_encode: n / len out of range");
  const int rows = n * len;
  for (int i = 0; i < rows; ++i)      // HF raises on such an id; the kernel's clamp stays as a guard only
    if (ids_host[i] < 0 || ids_host[i] >= TX_VOCAB) return m2t_set_error(M2T_ERR_ARG, "m2t_text_encode: input id outside [0, 28996)");
  hipStream_t st = (hipStream_t)stream;
  const int dt = p->dt;
  const float* wt = p->weights;
  const text_handles& hd = p->hd;
  const size_t es = p->lay.esz, hs_bytes = (size_t)rows * TX_H * es;
  char* W = (char*)workspace;
#define TX_KEEP_HIDDEN(i)                                                                                             \
  do {                                                                                                                \
    if (hidden_out) {                                                                                                 \
      hipError_t he = hipMemcpyAsync((char*)hidden_out + (size_t)(i) * hs_bytes, X, hs_bytes, hipMemcpyDeviceToDevice, st); \
      if (he != hipSuccess) return m2t_set_hip_error(he, __FILE__, __LINE__);                                         \
    }                                                                                                                 \
  } while (0)
  // a kernel templated on the element type T, at the handle's: the arguments may name T
#define TX_LAUNCH(kern, grid, block, ...)                                                                             \
  do {                                                                                                                \
    if (dt == M2T_F32) { using T = float; hipLaunchKernelGGL(kern<T>, grid, block, 0, st, __VA_ARGS__); }             \
    else { using T = bf16_t; hipLaunchKernelGGL(kern<T>, grid, block, 0, st, __VA_ARGS__); }                          \
    M2T_LAUNCH_CHECK();                                                                                               \
  } while (0)
  hipError_t e = hipMemcpyAsync(W + hd.ids, ids_host, sizeof(int) * rows, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(W + hd.mask, mask_host, sizeof(int) * rows, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);       // the host arrays may be temporaries
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  void *X = W + hd.X, *XM = W + hd.XM, *Y = W + hd.Y, *QKV = W + hd.QKV, *AO = W + hd.AO, *MH = W + hd.MH;
  float* pooled = (float*)(W + hd.pooled);
  const float* fbias = (const float*)(W + hd.fbias);
  const char* packed = W + hd.packed;
  const int* ids = (const int*)(W + hd.ids);
  const int* mask = (const int*)(W + hd.mask);
  TX_LAUNCH(text_embed_kernel, dim3((rows + 3) / 4), dim3(256), ids, wt + hd.word, wt + hd.pos, wt + hd.type, wt + hd.eln_w, wt + hd.eln_b,
            (T*)X, rows, len);
  TX_KEEP_HIDDEN(0);
  for (int l = 0; l < TX_LAYERS; ++l) {
    const text_layer& ly = hd.lyr[l];
    const m2t_tower_layer& L = ly.L;
    if (dt == M2T_F32) {      // the parity mode forms q | k | v with fp64 accumulation (see text_qkv_f64acc_kernel)
      static_assert((3 * TX_H) % 64 == 0 && TX_H % 16 == 0, "text_qkv_f64acc_kernel tiles");
      hipLaunchKernelGGL(text_qkv_f64acc_kernel, dim3(3 * TX_H / 64, (rows + 63) / 64), dim3(256), 0, st, (const float*)X,
                         (const float*)(packed + L.pk_qkv * es), fbias + L.fb_qkv, (float*)QKV, rows, 3 * TX_H, TX_H);
      M2T_LAUNCH_CHECK();
    } else {
      CK(tower_gemm(dt, M2T_E_BIAS, X, TX_H, packed + L.pk_qkv * es, QKV, 3 * TX_H, rows, fbias + L.fb_qkv, nullptr, st));
    }
    TX_LAUNCH(text_attn_kernel, dim3(n * TX_HEADS), dim3(256), (const T*)QKV, mask, (T*)AO, len);
    // BertSelfOutput: LayerNorm(dense(attention) + hidden); BertOutput: LayerNorm(dense(gelu(dense(h))) + h)
    CK(tower_gemm(dt, M2T_E_BIAS_RESID, AO, TX_H, packed + L.pk_o * es, Y, TX_H, rows, wt + L.o_b, X, st));
    CK(launch_layernorm(dt, Y, wt + ly.ln1_w, wt + ly.ln1_b, XM, rows, TX_H, st, 1e-12f));
    CK(tower_gemm(dt, M2T_E_BIAS_GELU, XM, TX_H, packed + L.pk_fc1 * es, MH, TX_FF, rows, wt + L.fc1_b, nullptr, st));
    CK(tower_gemm(dt, M2T_E_BIAS_RESID, MH, TX_FF, packed + L.pk_fc2 * es, Y, TX_H, rows, wt + L.fc2_b, XM, st));
    CK(launch_layernorm(dt, Y, wt + ly.ln2_w, wt + ly.ln2_b, X, rows, TX_H, st, 1e-12f));
    // hidden_states[l + 1] = X: the package pools hidden states 1, 2 and -1
    TX_KEEP_HIDDEN(l + 1);
    if (l == 0 || l == 1 || l == TX_LAYERS - 1) TX_LAUNCH(text_pool_kernel, dim3(n), dim3(256), (const T*)X, pooled, len, l == 0 ? 0 : 1);
  }
  hipLaunchKernelGGL(text_head_kernel, dim3(n), dim3(512), 0, st, pooled, wt + hd.head_w, emb);
  M2T_LAUNCH_CHECK();
#undef TX_LAUNCH
#undef TX_KEEP_HIDDEN
  return 0;
}
extern "C" int m2t_text_encode(m2t_text* p, const int* ids_host, const int* mask_host, int n, int len, float* emb, void* workspace,
                               void* stream) {
  return m2t_text_encode_ex(p, ids_host, mask_host, n, len, emb, workspace, stream, nullptr);
}
