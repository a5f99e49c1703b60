// m2t_swin.hip -- C ABI of the MedCLIP image tower (Swin-T 224) + the SemanticLoss value
// (include/m2t.h, "SemanticLoss" section).  Restates the arithmetic behind losses.py:53-79;
// forward only by default (the reference runs it under torch.no_grad()); the opt-in data gradient
// (m2t_swin_encode_grad / m2t_swin_backward) has its kernels in k_swin_bwd.hip.  Host code; forward
// kernels in k_swin.hip and k_gemm.hip.
#include "m2t_kernels.h"
#include "m2t_tower.h"
#include <cstring>
#include "../../include/m2t.h"
#include "../../include/m2t_swin.h"

namespace {
constexpr int DEPTHS[4] = {2, 2, 6, 2};
constexpr int HEADS[4] = {3, 6, 12, 24};
constexpr int MAX_DEPTH = 6;
static_assert(DEPTHS[0] <= MAX_DEPTH && DEPTHS[1] <= MAX_DEPTH && DEPTHS[2] <= MAX_DEPTH && DEPTHS[3] <= MAX_DEPTH, "blk[4][MAX_DEPTH]");
}

// ---- names resolved once: parameter offsets in floats, pack offsets in elements, workspace offsets in bytes ----
struct swin_block {
  m2t_tower_layer L;
  long long ln1_w, ln1_b, ln2_w, ln2_b, rel;   // parameters: layernorm_before / _after, relative-position bias table
  long long pk_fc1F, pk_fc2F;                  // packs of stages 0 / 1: fc1 / fc2 in MFMA fragment order (the fused MLP)
};
struct swin_merge { long long norm_w, norm_b, red_w, pk_red; };
struct swin_handles {                          // filled by m2t_swin_create
  swin_block blk[4][MAX_DEPTH];                // [stage][block < DEPTHS[stage]]
  swin_merge mrg[3];
  long long pe_w, pe_b, eln_w, eln_b, ln_w, ln_b, head_w, pk_pe;
  size_t packed, fbias, crops, A0, X, Hn, QKV, AO, MH;
};
struct swin_grad_block { size_t qkvT, oT, fc1T, fc2T, xin, xmid, qkv, gder; };
struct swin_grad_handles {                     // filled by grad_layout, for gws_n crops
  swin_grad_block blk[4][MAX_DEPTH];
  size_t redT[3], m[3];
  size_t gR, gF, gT, gC, gQ, gA, e0, xf, hnf, MD;
};

struct m2t_swin {
  int max_images, dt;
  m2t_layout lay;                          // names -> offsets: read by m2t_swin_query / m2t_swin_param_name only
  swin_handles hd;
  const float* weights = nullptr;          // caller's flat fp32 weights (device), set by load_weights
  // crop tables travel through a small ring of PINNED host slots, so the upload is a true asynchronous copy and the call returns
  // without waiting for the stream (round 3: the hipStreamSynchronize that protected a pageable temporary made every
  // SemanticLoss step wait for the model's forward pass -- 8 of the 11 ms of configs[2] were host stall)
  static constexpr int NPIN = 8;
  int* pinned = nullptr;                   // [NPIN][3 * max_images]
  hipEvent_t pin_ev[NPIN] = {};            // slot k's copy has been consumed
  bool pin_used[NPIN] = {};
  int pin_next = 0;
  // opt-in data gradient (m2t_swin_encode_grad / m2t_swin_backward): the grad workspace's layout for gws_n crops (names in gws for
  // the query keys, offsets in gh for the passes), the workspace whose transposed weights are current, and the crop count of the last stash
  m2t_region gws;
  swin_grad_handles gh;
  int gws_n = -1;
  const void* gws_packed = nullptr;
  int grad_n = 0;
  const void* grad_ws = nullptr;
  bool fused_mlp = true;                   // bf16, stages 1 / 2: LayerNorm + fc1 + GELU + fc2 + residual in one kernel (k_swin.hip)
};

extern "C" int m2t_swin_create(m2t_swin** out, int max_images, int dtype) {
  if (!out || max_images < 1 || (dtype != M2T_F32 && dtype != M2T_BF16)) return m2t_set_error(M2T_ERR_ARG, "m2t_swin_create: bad argument");
  m2t_swin* p = new m2t_swin();
  p->max_images = max_images; p->dt = dtype; p->lay.esz = (dtype == M2T_F32) ? 4 : 2;
  m2t_layout& lay = p->lay;
  swin_handles& hd = p->hd;
  // parameter inventory: HF swin-tiny checkpoint names (transformers 4.24), + the MedCLIP projection
  hd.pe_w = lay.add_param("embeddings.patch_embeddings.projection.weight", 96 * 48);
  hd.pe_b = lay.add_param("embeddings.patch_embeddings.projection.bias", 96);
  hd.eln_w = lay.add_param("embeddings.norm.weight", 96);
  hd.eln_b = lay.add_param("embeddings.norm.bias", 96);
  hd.pk_pe = lay.add_pack("pe", 96 * 48);
  for (int s = 0; s < 4; ++s) {
    const long long C = 96LL << s;
    for (int j = 0; j < DEPTHS[s]; ++j) {
      const std::string b = "encoder.layers." + std::to_string(s) + ".blocks." + std::to_string(j) + ".";
      swin_block& bk = hd.blk[s][j];
      bk.L.C = (int)C; bk.L.FF = (int)(4 * C);
      bk.ln1_w = lay.add_param(b + "layernorm_before.weight", C);
      bk.ln1_b = lay.add_param(b + "layernorm_before.bias", C);
      tower_add_qkv(lay, b, bk.L);
      bk.rel = lay.add_param(b + "attention.self.relative_position_bias_table", 169LL * HEADS[s]);
      tower_add_o(lay, b, bk.L);
      bk.ln2_w = lay.add_param(b + "layernorm_after.weight", C);
      bk.ln2_b = lay.add_param(b + "layernorm_after.bias", C);
      tower_add_mlp(lay, b, bk.L);
      tower_add_packs(lay, b, bk.L);
      bk.pk_fc1F = bk.pk_fc2F = -1;
      if (s < 2) { bk.pk_fc1F = lay.add_pack(b + "fc1F", 4 * C * C); bk.pk_fc2F = lay.add_pack(b + "fc2F", 4 * C * C); }   // MFMA fragment order: fused MLP of stages 1 / 2
    }
    if (s < 3) {
      const std::string d = "encoder.layers." + std::to_string(s) + ".downsample.";
      hd.mrg[s].norm_w = lay.add_param(d + "norm.weight", 4 * C);
      hd.mrg[s].norm_b = lay.add_param(d + "norm.bias", 4 * C);
      hd.mrg[s].red_w = lay.add_param(d + "reduction.weight", 8 * C * C);
      hd.mrg[s].pk_red = lay.add_pack(d + "red", 8 * C * C);
    }
  }
  hd.ln_w = lay.add_param("layernorm.weight", 768);
  hd.ln_b = lay.add_param("layernorm.bias", 768);
  hd.head_w = lay.add_param("projection_head.weight", 512 * 768);
  const size_t n = (size_t)max_images, es = lay.esz;
  const size_t tok = n * 3136 * 96;             // elements of the widest token tensor at every stage
  hd.packed = lay.ws.add("packed", (size_t)lay.npacked, es);
  hd.fbias = lay.ws.add("fbias", (size_t)lay.nfb, 4);
  hd.crops = lay.ws.add("crops", n * 3, 4);
  hd.A0 = lay.ws.add("A0", n * 3136 * 48, es);
  hd.X = lay.ws.add("X", tok, es);
  hd.Hn = lay.ws.add("Hn", tok, es);
  hd.QKV = lay.ws.add("QKV", tok * 3, es);
  hd.AO = lay.ws.add("AO", tok, es);
  hd.MH = lay.ws.add("MH", tok * 4, es);
  lay.ws.add("emb", n * 512, 4);
  lay.ws.seal();
  *out = p;
  return 0;
}
extern "C" void m2t_swin_destroy(m2t_swin* p) {
  if (!p) return;
  if (p->pinned) {
    (void)hipHostFree(p->pinned);
    for (auto& e : p->pin_ev) if (e) (void)hipEventDestroy(e);
  }
  delete p;
}
extern "C" long long m2t_swin_query(const m2t_swin* p, const char* key) {
  if (!p || !key) return -1;
  const std::string k(key);
  if (k == "max_images") return p->max_images;
  // grad workspace, in the layout of the last m2t_swin_grad_workspace_bytes(p, n_grad): byte offset / element count
  const bool goff = k.rfind("gws:", 0) == 0, gcnt = k.rfind("gwsn:", 0) == 0;
  if (goff || gcnt) {
    if (p->gws_n < 1) return -1;
    auto it = p->gws.t.find(k.substr(goff ? 4 : 5));
    if (it == p->gws.t.end()) return -1;
    return goff ? (long long)it->second.off : (long long)it->second.n;
  }
  return p->lay.query(k, m2t_layout::Q_WS | m2t_layout::Q_WSN);
}
// i-th parameter name in flat order (so the Python side never duplicates the inventory)
extern "C" const char* m2t_swin_param_name(const m2t_swin* p, int i) {
  return p ? p->lay.param_name(i) : nullptr;
}

// one-time: convert the frozen fp32 weights to the element type / fused layouts the kernels read
extern "C" int m2t_swin_load_weights(m2t_swin* p, const float* weights, void* workspace, void* stream) {
  if (!p || !weights || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_swin_load_weights: null");
  hipStream_t st = (hipStream_t)stream;
  const int dt = p->dt;
  const size_t es = p->lay.esz;
  const swin_handles& hd = p->hd;
  p->weights = weights;
  p->gws_packed = nullptr;                 // the transposed weights of a grad workspace are re-derived on its next use
  char* packed = (char*)workspace + hd.packed;
  float* fbias = (float*)((char*)workspace + hd.fbias);
  CK(launch_convert(dt, weights + hd.pe_w, packed + hd.pk_pe * es, 96 * 48, st));
  for (int s = 0; s < 4; ++s) {
    const long long C = 96LL << s;
    for (int j = 0; j < DEPTHS[s]; ++j) {
      const swin_block& bk = hd.blk[s][j];
      CK(tower_pack_layer(dt, es, bk.L, weights, packed, fbias, st));
      if (s < 2) {
        CK(launch_frag16_pack(dt, weights + bk.L.fc1_w, packed + bk.pk_fc1F * es, (int)(4 * C), (int)C, st));
        CK(launch_frag16_pack(dt, weights + bk.L.fc2_w, packed + bk.pk_fc2F * es, (int)C, (int)(4 * C), st));
      }
    }
    if (s < 3) CK(launch_convert(dt, weights + hd.mrg[s].red_w, packed + hd.mrg[s].pk_red * es, 8 * C * C, st));
  }
  return 0;
}

// ---- opt-in data gradient: grad workspace layout -------------------------------------------------------------------------
// [transposed weights of the data-gradient GEMMs | fp32 scratch of the backward | stash of n_grad crops | gelu' of the forward]
// stash per crop (elements of the storage type): e0 = 3136 x 96 (embedding before its LayerNorm); per block of stage s
// (T_s = 3136 / 4^s tokens, C_s = 96 2^s): xin, xmid (the two LayerNorm inputs) 2 T_s C_s, qkv 3 T_s C_s, gelu'(fc1) 4 T_s C_s;
// per patch merging the gathered rows T_s C_s; the final LayerNorm's input and output 2 x 49 x 768.  13.7 M elements per crop.
// Names (the gws: / gwsn: query keys) and the offsets the passes index (p->gh) are laid together, once per crop count.
static void grad_layout(m2t_swin* p, int ng) {
  if (p->gws_n == ng) return;
  m2t_region& gws = p->gws;
  swin_grad_handles& gh = p->gh;
  gws.clear();
  const size_t es = p->lay.esz, g = (size_t)ng, tok = g * 3136 * 96;
  for (int s = 0; s < 4; ++s) {
    const size_t C = 96u << s;
    for (int j = 0; j < DEPTHS[s]; ++j) {
      const std::string b = "encoder.layers." + std::to_string(s) + ".blocks." + std::to_string(j) + ".";
      swin_grad_block& gb = gh.blk[s][j];
      gb.qkvT = gws.add(b + "qkvT", 3 * C * C, es);
      gb.oT = gws.add(b + "oT", C * C, es);
      gb.fc1T = gws.add(b + "fc1T", 4 * C * C, es);
      gb.fc2T = gws.add(b + "fc2T", 4 * C * C, es);
    }
    if (s < 3) gh.redT[s] = gws.add("encoder.layers." + std::to_string(s) + ".downsample.redT", 8 * C * C, es);
  }
  gh.gR = gws.add("gR", tok, 4);            // residual-stream gradient (fp32 in both modes)
  gh.gF = gws.add("gF", tok, 4);            // fp32 LayerNorm-gradient scratch (merge, embedding)
  gh.gT = gws.add("gT", tok, es);           // storage-type copy of gR: the operand of the next data-gradient GEMM
  gh.gC = gws.add("gC", tok, es);
  gh.gQ = gws.add("gQ", tok * 3, es);
  gh.gA = gws.add("gA", tok * 4, es);
  gh.e0 = gws.add("e0", tok, es);
  for (int s = 0; s < 4; ++s) {
    const size_t tc = tok >> s;        // tokens x channels of stage s
    for (int j = 0; j < DEPTHS[s]; ++j) {
      const std::string b = "s" + std::to_string(s) + "b" + std::to_string(j) + ".";
      swin_grad_block& gb = gh.blk[s][j];
      gb.xin = gws.add(b + "xin", tc, es);
      gb.xmid = gws.add(b + "xmid", tc, es);
      gb.qkv = gws.add(b + "qkv", 3 * tc, es);
      gb.gder = gws.add(b + "gder", 4 * tc, es);
    }
    if (s < 3) gh.m[s] = gws.add("m" + std::to_string(s), tc, es);
  }
  gh.xf = gws.add("xf", g * 49 * 768, es);
  gh.hnf = gws.add("hnf", g * 49 * 768, es);
  gh.MD = gws.add("MD", (size_t)p->max_images * 3136 * 96 * 4, es);   // gelu'(fc1) of every crop of the call (stash keeps the first n_grad)
  gws.seal();
  p->gws_n = ng;
}

extern "C" long long m2t_swin_grad_workspace_bytes(m2t_swin* p, int n_grad) {
  if (!p || n_grad < 1 || n_grad > p->max_images) return m2t_set_error(M2T_ERR_ARG, "m2t_swin_grad_workspace_bytes: n_grad out of range");
  grad_layout(p, n_grad);
  return (long long)p->gws.bytes;
}

static int pack_grad_weights(m2t_swin* p, void* grad_ws, hipStream_t st) {
  const int dt = p->dt;
  const float* wt = p->weights;
  char* gw = (char*)grad_ws;
  for (int s = 0; s < 4; ++s) {
    const int C = 96 << s;
    for (int j = 0; j < DEPTHS[s]; ++j) {
      const m2t_tower_layer& L = p->hd.blk[s][j].L;
      const swin_grad_block& gb = p->gh.blk[s][j];
      for (int part = 0; part < 3; ++part) CK(launch_transpose_convert(dt, wt + L.w[part], gw + gb.qkvT, C, C, 3 * C, C * part, st));
      CK(launch_transpose_convert(dt, wt + L.o_w, gw + gb.oT, C, C, C, 0, st));
      CK(launch_transpose_convert(dt, wt + L.fc1_w, gw + gb.fc1T, 4 * C, C, 4 * C, 0, st));
      CK(launch_transpose_convert(dt, wt + L.fc2_w, gw + gb.fc2T, C, 4 * C, C, 0, st));
    }
    if (s < 3) CK(launch_transpose_convert(dt, wt + p->hd.mrg[s].red_w, gw + p->gh.redT[s], 2 * C, 4 * C, 2 * C, 0, st));
  }
  p->gws_packed = grad_ws;
  return 0;
}

// encode n (<= max_images) 224x224 crops of the source images in TWO tensors (indices 0 .. n_a - 1 in src, n_a .. n_a + n_b - 1 in
// src_b; n_b may be 0): crops_host [n][3] = (source index, y0, x0) -> emb [n][512] (unit norm, fp32, device).  grad_ws (nullable):
// also keep what the backward needs of the first n_grad crops; hidden_out (nullable): also copy the stage inputs of all n crops
static int encode_impl(m2t_swin* p, const float* src, int n_a, const float* src_b, int n_b, int Hs, int Ws, const int* crops_host, int n,
                       float* emb, void* workspace, int n_grad, void* grad_ws, void* hidden_out, hipStream_t st) {
  const int n_src = n_a + n_b;
  if (!p || !src || !crops_host || !emb || !workspace || n_a < 1 || n_b < 0 || (n_b > 0 && !src_b))
    return m2t_set_error(M2T_ERR_ARG, "m2t_swin_encode: null / bad source counts");
  if (!p->weights) return m2t_set_error(M2T_ERR_STATE, "m2t_swin_encode: call m2t_swin_load_weights first");
  if (n < 1 || n > p->max_images) return m2t_set_error(M2T_ERR_ARG, "m2t_swin_encode: n out of range");
  for (int i = 0; i < n; ++i) {
    const int si = crops_host[3 * i], y0 = crops_host[3 * i + 1], x0 = crops_host[3 * i + 2];
    if (si < 0 || si >= n_src || y0 < 0 || x0 < 0 || y0 + 224 > Hs || x0 + 224 > Ws)
      return m2t_set_error(M2T_ERR_ARG, "m2t_swin_encode: crop outside its source image");
  }
  const bool G = grad_ws != nullptr;
  if (G) {
    grad_layout(p, n_grad);
    if (p->gws_packed != grad_ws) CK(pack_grad_weights(p, grad_ws, st));
    p->grad_n = 0;                     // until the stash below is complete
    p->grad_ws = grad_ws;
  }
  const swin_handles& hd = p->hd;
  const swin_grad_handles& gh = p->gh;   // (read in grad mode only)
  const size_t es = p->lay.esz;
  char* gw = (char*)grad_ws;
  // grad mode: the first n_grad crops' copy of a token tensor (contiguous rows at the front of the batch) into the stash at byte
  // offset `to` of the grad workspace
  // hidden_out (m2t_swin_encode_ex): all n crops' copy, the tensors one after the other in the order of the calls below
  size_t hcur = 0;
  auto stash = [&](const void* from, size_t to, size_t elems_per_crop) -> int {
    if (hidden_out) {
      const size_t nb = elems_per_crop * n * es;
      const hipError_t e1 = hipMemcpyAsync((char*)hidden_out + hcur, from, nb, hipMemcpyDeviceToDevice, st);
      if (e1 != hipSuccess) return m2t_set_hip_error(e1, __FILE__, __LINE__);
      hcur += nb;
    }
    if (!G) return 0;
    const hipError_t e2 = hipMemcpyAsync(gw + to, from, elems_per_crop * n_grad * es, hipMemcpyDeviceToDevice, st);
    return e2 == hipSuccess ? 0 : m2t_set_hip_error(e2, __FILE__, __LINE__);
  };
  const int dt = p->dt;
  const float* wt = p->weights;
  hipError_t e = hipSuccess;
  if (!p->pinned) {
    e = hipHostMalloc((void**)&p->pinned, sizeof(int) * 3 * (size_t)p->max_images * m2t_swin::NPIN, hipHostMallocDefault);
    if (e != hipSuccess) { p->pinned = nullptr; return m2t_set_hip_error(e, __FILE__, __LINE__); }
    for (auto& ev : p->pin_ev) {
      e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
    }
  }
  char* W = (char*)workspace;
  const int slot = p->pin_next;
  p->pin_next = (slot + 1) % m2t_swin::NPIN;
  if (p->pin_used[slot]) {             // eight encodes ago: long done unless the caller never synchronises
    e = hipEventSynchronize(p->pin_ev[slot]);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  }
  int* stage = p->pinned + (size_t)slot * 3 * p->max_images;
  memcpy(stage, crops_host, sizeof(int) * 3 * n);      // crops_host may be a temporary of the caller
  e = hipMemcpyAsync(W + hd.crops, stage, sizeof(int) * 3 * n, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  e = hipEventRecord(p->pin_ev[slot], st);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  p->pin_used[slot] = true;
  void *X = W + hd.X, *Hn = W + hd.Hn, *QKV = W + hd.QKV, *AO = W + hd.AO, *MH = W + hd.MH;
  const float* fbias = (const float*)(W + hd.fbias);
  const char* packed = W + hd.packed;
  CK(launch_swin_patchify(dt, src, src_b, n_a, Hs, Ws, (const int*)(W + hd.crops), n, W + hd.A0, st));
  long long M = (long long)n * 3136;
  CK(tower_gemm(dt, M2T_E_BIAS, W + hd.A0, 48, packed + hd.pk_pe * es, X, 96, M, wt + hd.pe_b, nullptr, st));
  CK(stash(X, gh.e0, 3136 * 96));
  CK(launch_layernorm(dt, X, wt + hd.eln_w, wt + hd.eln_b, X, M, 96, st));
  int H = 56;
  for (int s = 0; s < 4; ++s) {
    const int C = 96 << s;
    for (int j = 0; j < DEPTHS[s]; ++j) {
      const swin_block& bk = hd.blk[s][j];
      const m2t_tower_layer& L = bk.L;
      const swin_grad_block& gb = gh.blk[s][j];
      const int shift = (j % 2 == 0 || H <= 7) ? 0 : 3;
      const size_t tc = (size_t)(H * H) * C;
      CK(stash(X, gb.xin, tc));
      CK(launch_layernorm(dt, X, wt + bk.ln1_w, wt + bk.ln1_b, Hn, M, C, st));
      CK(tower_gemm(dt, M2T_E_BIAS, Hn, C, packed + L.pk_qkv * es, QKV, 3 * C, M, fbias + L.fb_qkv, nullptr, st));
      CK(stash(QKV, gb.qkv, 3 * tc));
      CK(launch_swin_attn(dt, QKV, wt + bk.rel, AO, n, H, H, C, HEADS[s], shift, st));
      CK(tower_gemm(dt, M2T_E_BIAS_RESID, AO, C, packed + L.pk_o * es, X, C, M, wt + L.o_b, X, st));
      CK(stash(X, gb.xmid, tc));
      if (G) {
        // fc1 + bias + GELU storing gelu'(t) beside gelu(t) (the bias / GELU / derivative epilogue of gemm_nt with a trivial
        // 1 x 1 shuffle; fp32: the same accumulation and the same erf GELU as M2T_E_BIAS_GELU, so emb is bit-identical)
        CK(launch_layernorm(dt, X, wt + bk.ln2_w, wt + bk.ln2_b, Hn, M, C, st));
        m2t_gemm_args ga{};
        ga.A = Hn; ga.lda = C; ga.W = packed + L.pk_fc1 * es; ga.Y = MH; ga.ldy = 4 * C; ga.Y2 = gw + gh.MD;
        ga.bias = wt + L.fc1_b; ga.M = M; ga.N = 4 * C; ga.K = C;
        ga.H = 1; ga.Wd = 1; ga.r = 1; ga.C = 4 * C;
        CK(launch_gemm_nt(dt, M2T_A_PLAIN, M2T_E_BIAS_SHUF, ga, st));
        CK(stash(gw + gh.MD, gb.gder, 4 * tc));
        CK(tower_gemm(dt, M2T_E_BIAS_RESID, MH, 4 * C, packed + L.pk_fc2 * es, X, C, M, wt + L.fc2_b, X, st));
        continue;
      }
      if (dt != M2T_F32 && s < 2 && p->fused_mlp) {
        // LayerNorm + fc1 + GELU + fc2 + residual in one kernel: the 4C-wide hidden tensor stays in LDS
        CK(launch_swin_mlp_fused(X, wt + bk.ln2_w, wt + bk.ln2_b, packed + bk.pk_fc1F * es, wt + L.fc1_b, packed + bk.pk_fc2F * es,
                                  wt + L.fc2_b, M, C, st));
        continue;
      }
      CK(launch_layernorm(dt, X, wt + bk.ln2_w, wt + bk.ln2_b, Hn, M, C, st));
      CK(tower_gemm(dt, M2T_E_BIAS_GELU, Hn, C, packed + L.pk_fc1 * es, MH, 4 * C, M, wt + L.fc1_b, nullptr, st));
      CK(tower_gemm(dt, M2T_E_BIAS_RESID, MH, 4 * C, packed + L.pk_fc2 * es, X, C, M, wt + L.fc2_b, X, st));
    }
    if (s < 3) {
      const swin_merge& mg = hd.mrg[s];
      CK(launch_swin_merge_gather(dt, X, Hn, n, H, H, C, st));
      CK(stash(Hn, gh.m[s], (size_t)(H * H) * C));
      M /= 4; H /= 2;
      CK(launch_layernorm(dt, Hn, wt + mg.norm_w, wt + mg.norm_b, Hn, M, 4 * C, st));
      CK(tower_gemm(dt, M2T_E_PLAIN, Hn, 4 * C, packed + mg.pk_red * es, X, 2 * C, M, nullptr, nullptr, st));
    }
  }
  CK(stash(X, gh.xf, 49 * 768));
  CK(launch_layernorm(dt, X, wt + hd.ln_w, wt + hd.ln_b, Hn, M, 768, st));
  CK(stash(Hn, gh.hnf, 49 * 768));
  CK(launch_swin_head(dt, Hn, wt + hd.head_w, emb, n, st));
  if (G) p->grad_n = n_grad;
  return 0;
}

// m2t_swin_encode_pair that also copies the stage inputs of all n crops to hidden_out (include/m2t_swin.h has the order); the copies
// are device-to-device on the call's stream between the launches, which are those of the plain call
extern "C" int m2t_swin_encode_ex(m2t_swin* p, const float* src, int n_a, const float* src_b, int n_b, int Hs, int Ws,
                                  const int* crops_host, int n, float* emb, void* workspace, void* stream, void* hidden_out) {
  return encode_impl(p, src, n_a, src_b, n_b, Hs, Ws, crops_host, n, emb, workspace, 0, nullptr, hidden_out, (hipStream_t)stream);
}
// the sources in one tensor: src [n_src][3][Hs][Ws] fp32 NCHW (device)
extern "C" int m2t_swin_encode(m2t_swin* p, const float* src, int n_src, int Hs, int Ws, const int* crops_host, int n,
                               float* emb, void* workspace, void* stream) {
  return m2t_swin_encode_ex(p, src, n_src, nullptr, 0, Hs, Ws, crops_host, n, emb, workspace, stream, nullptr);
}
// the SR and HR batches of SemanticLoss.batch are encoded in one pass without concatenating them first
extern "C" int m2t_swin_encode_pair(m2t_swin* p, const float* src, int n_a, const float* src_b, int n_b, int Hs, int Ws,
                                    const int* crops_host, int n, float* emb, void* workspace, void* stream) {
  return m2t_swin_encode_ex(p, src, n_a, src_b, n_b, Hs, Ws, crops_host, n, emb, workspace, stream, nullptr);
}
extern "C" int m2t_swin_encode_grad(m2t_swin* p, const float* src_a, int n_a, const float* src_b, int n_b, int Hs, int Ws,
                                    const int* crops_host, int n, int n_grad, float* emb, void* workspace, void* grad_ws, void* stream) {
  if (!p || !grad_ws) return m2t_set_error(M2T_ERR_ARG, "m2t_swin_encode_grad: null");
  if (n_grad < 1 || n_grad > n) return m2t_set_error(M2T_ERR_ARG, "m2t_swin_encode_grad: n_grad must be in [1, n]");
  return encode_impl(p, src_a, n_a, src_b, n_b, Hs, Ws, crops_host, n, emb, workspace, n_grad, grad_ws, nullptr, (hipStream_t)stream);
}

// vector-Jacobian product of encode_image for the n_grad crops stashed by the last m2t_swin_encode_grad:
// g_emb [n_grad,512] -> g_crops [n_grad,3,224,224] fp32 (overwritten)
extern "C" int m2t_swin_backward(m2t_swin* p, const float* g_emb, int n_grad, float* g_crops, void* workspace, void* grad_ws, void* stream) {
  return m2t_swin_backward_ex(p, g_emb, n_grad, g_crops, workspace, grad_ws, stream, nullptr);
}
// the same, with the fp32 residual-stream gradient copied to grad_taps after every step that completes it (include/m2t.h has
// the order); device-to-device copies on the call's stream between the launches of the plain call
extern "C" int m2t_swin_backward_ex(m2t_swin* p, const float* g_emb, int n_grad, float* g_crops, void* workspace, void* grad_ws, void* stream,
                                    float* grad_taps) {
  if (!p || !g_emb || !g_crops || !workspace || !grad_ws) return m2t_set_error(M2T_ERR_ARG, "m2t_swin_backward: null");
  if (!p->weights) return m2t_set_error(M2T_ERR_STATE, "m2t_swin_backward: call m2t_swin_load_weights first");
  if (p->grad_n < 1 || p->grad_n != n_grad || p->grad_ws != grad_ws || p->gws_packed != grad_ws)
    return m2t_set_error(M2T_ERR_STATE, "m2t_swin_backward: needs m2t_swin_encode_grad with the same n_grad and grad workspace first");
  grad_layout(p, n_grad);
  hipStream_t st = (hipStream_t)stream;
  const int dt = p->dt;
  const float* wt = p->weights;
  const swin_handles& hd = p->hd;
  const swin_grad_handles& gh = p->gh;
  char* gw = (char*)grad_ws;
  float *gR = (float*)(gw + gh.gR), *gF = (float*)(gw + gh.gF);
  void *gT = gw + gh.gT, *gC = gw + gh.gC, *gQ = gw + gh.gQ, *gA = gw + gh.gA;
  const int ng = n_grad;
  size_t tcur = 0;
  auto tap = [&](const float* from, size_t elems) -> int {
    if (!grad_taps) return 0;
    const hipError_t e1 = hipMemcpyAsync(grad_taps + tcur, from, elems * sizeof(float), hipMemcpyDeviceToDevice, st);
    tcur += elems;
    return e1 == hipSuccess ? 0 : m2t_set_hip_error(e1, __FILE__, __LINE__);
  };
  CK(launch_swin_head_bwd(dt, gw + gh.hnf, wt + hd.head_w, g_emb, gC, ng, st));
  CK(launch_layernorm_bwd(dt, gw + gh.xf, gC, wt + hd.ln_w, nullptr, gR, gT, (long long)ng * 49, 768, st));
  CK(tap(gR, (size_t)ng * 49 * 768));
  for (int s = 3; s >= 0; --s) {
    const int H = 56 >> s, C = 96 << s;
    const long long M = (long long)ng * H * H;
    for (int j = DEPTHS[s] - 1; j >= 0; --j) {
      const swin_block& bk = hd.blk[s][j];
      const swin_grad_block& gb = gh.blk[s][j];
      const int shift = (j % 2 == 0 || H <= 7) ? 0 : 3;
      // MLP: d(fc1 out) = (g W2) o gelu'(t); d(LN2 out) = that W1; + LayerNorm backward into the residual stream
      CK(tower_gemm(dt, M2T_E_GELU_GRAD, gT, C, gw + gb.fc2T, gA, 4 * C, M, nullptr, gw + gb.gder, st));
      CK(tower_gemm(dt, M2T_E_PLAIN, gA, 4 * C, gw + gb.fc1T, gC, C, M, nullptr, nullptr, st));
      CK(launch_layernorm_bwd(dt, gw + gb.xmid, gC, wt + bk.ln2_w, gR, gR, gT, M, C, st));
      CK(tap(gR, (size_t)M * C));
      // attention: o_proj^T, window attention, qkv^T, LayerNorm backward into the residual stream
      CK(tower_gemm(dt, M2T_E_PLAIN, gT, C, gw + gb.oT, gC, C, M, nullptr, nullptr, st));
      CK(launch_swin_attn_bwd(dt, gw + gb.qkv, wt + bk.rel, gC, gQ, ng, H, H, C, HEADS[s], shift, st));
      CK(tower_gemm(dt, M2T_E_PLAIN, gQ, 3 * C, gw + gb.qkvT, gC, C, M, nullptr, nullptr, st));
      CK(launch_layernorm_bwd(dt, gw + gb.xin, gC, wt + bk.ln1_w, gR, gR, gT, M, C, st));
      CK(tap(gR, (size_t)M * C));
    }
    if (s > 0) {
      // patch merging of stage s - 1 (C' = C / 2 channels at 2H x 2H): reduction^T, LayerNorm backward (4 C'), scatter
      CK(tower_gemm(dt, M2T_E_PLAIN, gT, C, gw + gh.redT[s - 1], gC, 2 * C, M, nullptr, nullptr, st));
      CK(launch_layernorm_bwd(dt, gw + gh.m[s - 1], gC, wt + hd.mrg[s - 1].norm_w, nullptr, gF, nullptr, M, 2 * C, st));
      CK(launch_swin_merge_scatter(dt, gF, gR, gT, ng, 2 * H, 2 * H, C / 2, st));
      CK(tap(gR, (size_t)M * 2 * C));
    }
  }
  // embedding LayerNorm (its incoming gradient is the fp32 residual stream) and the patch projection^T + patchify adjoint, fp32
  CK(launch_layernorm_bwd(dt, gw + gh.e0, nullptr, wt + hd.eln_w, nullptr, gF, nullptr, (long long)ng * 3136, 96, st, 1e-5f, gR));
  CK(tap(gF, (size_t)ng * 3136 * 96));
  CK(launch_swin_embed_bwd(gF, wt + hd.pe_w, g_crops, ng, st));
  return 0;
}

extern "C" int m2t_semantic_loss_backward(const float* emb, const float* text, int B, int n_patches, float* g_emb, void* stream) {
  if (!emb || !text || !g_emb || B < 1 || n_patches < 1) return m2t_set_error(M2T_ERR_ARG, "m2t_semantic_loss_backward: bad argument");
  return launch_semantic_loss_bwd(emb, text, B, n_patches, g_emb, (hipStream_t)stream);
}
extern "C" int m2t_bicubic_resize_backward(const float* g_dst, float* g_src, int NC, int Hin, int Win, int Hout, int Wout, void* stream) {
  if (!g_dst || !g_src || NC < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1)
    return m2t_set_error(M2T_ERR_ARG, "m2t_bicubic_resize_backward: bad argument");
  return launch_bicubic_resize_bwd(g_dst, g_src, NC, Hin, Win, Hout, Wout, (hipStream_t)stream);
}

extern "C" int m2t_semantic_loss(const float* emb, const float* text, int B, int n_patches, float* per_sample, float* total,
                                 void* stream) {
  if (!emb || !text || B < 1 || n_patches < 1) return m2t_set_error(M2T_ERR_ARG, "m2t_semantic_loss: bad argument");
  return launch_semantic_loss(emb, text, B, n_patches, per_sample, total, (hipStream_t)stream);
}
extern "C" int m2t_bicubic_resize(const float* src, float* dst, int NC, int Hin, int Win, int Hout, int Wout, void* stream) {
  if (!src || !dst || NC < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1) return m2t_set_error(M2T_ERR_ARG, "m2t_bicubic_resize: bad argument");
  return launch_bicubic_resize(src, dst, NC, Hin, Win, Hout, Wout, (hipStream_t)stream);
}
