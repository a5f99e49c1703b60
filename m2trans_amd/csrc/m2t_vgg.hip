// m2t_vgg.hip -- C ABI of the VGG19 feature loss (include/m2t_perceptual.h): the tower object, the workspace layout, the loss routine
// behind m2t_vgg_loss_tensor and m2t_vgg_loss (m2t_api.hip), and the operator entries.  Host code; kernels in k_vgg.hip.
#include "m2t_kernels.h"
#include "m2t_layout.h"
#include <cmath>
#include <cstring>
#include "../../include/m2t_perceptual.h"

namespace {
constexpr int NL = 13, NTAP = 5;
const int CIN[NL] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
const int COUT[NL] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512};
const int FEAT[NL] = {0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28};     // torchvision vgg19: features.<i>
const int LEVEL[NL] = {0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4};             // pools before the layer
const int TAP_LAYER[NTAP] = {0, 2, 4, 8, 12};
constexpr int MIN_SIDE = 16, MAX_B = 32767, PART = 256;

int tap_of(int l) { for (int k = 0; k < NTAP; ++k) if (TAP_LAYER[k] == l) return k; return -1; }
bool pool_before(int l) { return l > 0 && LEVEL[l] != LEVEL[l - 1]; }

struct VggLayout {          // byte offsets inside the workspace
  int h[5], w[5];
  size_t act[NL], pooled[5], ytap[NTAP], part, pp[2], g[NL], gp, bytes_value, bytes_grad;
  size_t elems(int B, int l) const { return (size_t)B * h[LEVEL[l]] * w[LEVEL[l]] * COUT[l]; }
};

bool vgg_layout(int B, int H, int W, VggLayout& L) {
  if (B < 1 || B > MAX_B || H < MIN_SIDE || W < MIN_SIDE) return false;
  for (int s = 0; s < 5; ++s) { L.h[s] = H >> s; L.w[s] = W >> s; }
  size_t off = 0;
  auto add = [&off](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  for (int l = 0; l < NL; ++l) L.act[l] = add(L.elems(B, l) * 2);
  L.pooled[0] = 0;
  for (int s = 1; s < 5; ++s) L.pooled[s] = add((size_t)B * L.h[s] * L.w[s] * (64 << (s - 1)) * 2);
  for (int k = 0; k < NTAP; ++k) L.ytap[k] = add(L.elems(B, TAP_LAYER[k]) * 2);
  L.part = add(sizeof(double) * NTAP * PART);
  L.pp[0] = add(L.elems(B, 0) * 2);
  L.pp[1] = add(L.elems(B, 0) * 2);
  L.bytes_value = off;
  for (int l = 0; l < NL; ++l) L.g[l] = add(L.elems(B, l) * 2);
  L.gp = add((size_t)B * L.h[1] * L.w[1] * 64 * 2);
  L.bytes_grad = off;
  return true;
}
}  // namespace

struct m2t_vgg {
  m2t_layout lay;
  const char* packed = nullptr;            // the caller's device buffer, set by load_weights
  size_t wf[NL] = {}, wb[NL] = {}, w0 = 0, bias[NL] = {}, packed_bytes = 0;     // byte offsets inside it
  long long pw[NL] = {}, pb[NL] = {};      // each layer's weight and bias in the flat fp32 parameters (offsets in floats)
};

extern "C" int m2t_vgg_create(m2t_vgg** out, int dtype) {
  if (!out) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_create: null");
  if (dtype == M2T_F32) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_create: the VGG19 tower computes in bf16 only (dtype M2T_BF16); fp32 is not built");
  if (dtype != M2T_BF16) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_create: unknown dtype");
  m2t_vgg* v = new m2t_vgg();
  size_t off = 0;
  auto add = [&off](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
  for (int l = 0; l < NL; ++l) {
    const std::string b = "features." + std::to_string(FEAT[l]) + ".";
    v->pw[l] = v->lay.add_param(b + "weight", (long long)COUT[l] * CIN[l] * 9);
    v->pb[l] = v->lay.add_param(b + "bias", COUT[l]);
    if (l == 0) {
      v->w0 = add(27 * 64 * 4);
    } else {
      v->wf[l] = add((size_t)COUT[l] * CIN[l] * 9 * 2);
      v->wb[l] = add((size_t)COUT[l] * CIN[l] * 9 * 2);
    }
    v->bias[l] = add((size_t)COUT[l] * 4);
  }
  v->packed_bytes = off;
  *out = v;
  return 0;
}
extern "C" void m2t_vgg_destroy(m2t_vgg* v) { delete v; }
extern "C" long long m2t_vgg_query(const m2t_vgg* v, const char* key) {
  if (!v || !key) return -1;
  const std::string k(key);
  if (k == "packed_bytes") return (long long)v->packed_bytes;
  if (k == "loaded") return v->packed ? 1 : 0;
  if (k == "workspace_bytes") return -1;     // depends on the shape: m2t_vgg_workspace_bytes
  return v->lay.query(k, 0);
}
extern "C" const char* m2t_vgg_param_name(const m2t_vgg* v, int i) { return v ? v->lay.param_name(i) : nullptr; }

extern "C" int m2t_vgg_load_weights(m2t_vgg* v, const float* weights, void* packed, void* stream) {
  if (!v || !weights || !packed) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_load_weights: null");
  hipStream_t st = (hipStream_t)stream;
  char* pk = (char*)packed;
  for (int l = 0; l < NL; ++l) {
    const float* w = weights + v->pw[l];
    if (l == 0) {
      CK(launch_vgg_pack_first(w, (float*)(pk + v->w0), st));
    } else {
      CK(launch_vgg_pack(w, pk + v->wf[l], COUT[l], CIN[l], 0, st));
      CK(launch_vgg_pack(w, pk + v->wb[l], COUT[l], CIN[l], 1, st));
    }
    CK(launch_convert(M2T_F32, weights + v->pb[l], pk + v->bias[l], COUT[l], st));
  }
  v->packed = pk;
  return 0;
}

extern "C" size_t m2t_vgg_workspace_bytes(int B, int H, int W, int want_grad) {
  VggLayout L;
  if (!vgg_layout(B, H, W, L)) return 0;
  return want_grad ? L.bytes_grad : L.bytes_value;
}
extern "C" size_t m2t_vgg_workspace_offset(int B, int H, int W, int region, int index) {
  VggLayout L;
  if (!vgg_layout(B, H, W, L) || index < 0) return (size_t)-1;
  if (region == 0 && index < NL) return L.act[index];
  if (region == 1 && index < NTAP) return L.ytap[index];
  if (region == 2 && index < NTAP) return L.part + sizeof(double) * PART * index;
  if (region == 3 && index < NL) return L.g[index];
  return (size_t)-1;
}

namespace {
struct VggSrc { const float* x; long long img, chs; int row; float R; int clamp; };

// the tower on one half: act[l] receives the post-ReLU output of layer l, pooled[s] the input of level s
int vgg_forward(const m2t_vgg* v, const VggSrc& s, int B, const VggLayout& L, void* const* act, void* const* pooled, hipStream_t st) {
  const M2TPixelLoss none;
  CK(launch_vgg_first_fwd(s.x, s.img, s.chs, s.row, s.R, s.clamp, (const float*)(v->packed + v->w0), (const float*)(v->packed + v->bias[0]),
                          act[0], B, L.h[0], L.w[0], st));
  for (int l = 1; l < NL; ++l) {
    const int lv = LEVEL[l];
    const void* in = act[l - 1];
    if (pool_before(l)) {
      CK(launch_vgg_pool_fwd(act[l - 1], pooled[lv], B, L.h[lv - 1], L.w[lv - 1], COUT[l - 1], st));
      in = pooled[lv];
    }
    CK(launch_vgg_conv(0, in, v->packed + v->wf[l], act[l], B, L.h[lv], L.w[lv], CIN[l], COUT[l], (const float*)(v->packed + v->bias[l]),
                       nullptr, nullptr, none, st));
  }
  return 0;
}
}  // namespace

// the one device routine behind m2t_vgg_loss_tensor and m2t_vgg_loss (arguments checked by the callers): tap k's mean divides by
// divisor * C_k H_k W_k
int launch_vgg_loss(const m2t_vgg* v, const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R,
                    int clamp, int kind, float param, const double* tw, double scale, double divisor, float* gx_add, float* loss_out,
                    double* per_tap_out, int accumulate, void* workspace, hipStream_t st) {
  VggLayout L;
  if (!vgg_layout(B, H, W, L)) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss: unsupported shape");
  M2TPixelLoss value;
  if (!m2t_pixel_loss_make(kind, param, 1.f, &value)) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss: unknown kind, or eps / beta not finite and > 0");
  char* ws = (char*)workspace;
  void *xa[NL], *xp[5] = {}, *ya[NL], *yp[5] = {};
  for (int l = 0; l < NL; ++l) xa[l] = ws + L.act[l];
  for (int s = 1; s < 5; ++s) xp[s] = ws + L.pooled[s];
  // the y half keeps only its taps: everything else alternates between two buffers
  void* pp[2] = {ws + L.pp[0], ws + L.pp[1]};
  const void* last = nullptr;
  auto pick = [&]() { void* b = (last == pp[0]) ? pp[1] : pp[0]; last = b; return b; };
  for (int l = 0; l < NL; ++l) {
    if (pool_before(l)) yp[LEVEL[l]] = pick();
    const int k = tap_of(l);
    if (k >= 0) { ya[l] = ws + L.ytap[k]; last = ya[l]; } else ya[l] = pick();
  }
  const VggSrc sy{y, (long long)C * H * W, C == 1 ? 0LL : (long long)H * W, W, R, 0};
  const VggSrc sx{x, xs_img, C == 1 ? 0LL : xs_img / C, xs_row, R, clamp};
  CK(vgg_forward(v, sy, B, L, ya, yp, st));
  CK(vgg_forward(v, sx, B, L, xa, xp, st));

  double* part = (double*)(ws + L.part);
  int nblk[NTAP];
  double wn[NTAP], inv_n[NTAP];
  M2TPixelLoss seed[NTAP];
  for (int k = 0; k < NTAP; ++k) {
    const int l = TAP_LAYER[k];
    const long long n = (long long)L.elems(B, l);
    inv_n[k] = 1.0 / (divisor * (double)COUT[l] * L.h[LEVEL[l]] * L.w[LEVEL[l]]);
    wn[k] = scale * tw[k] * inv_n[k];
    nblk[k] = vgg_tap_blocks(n);
    if (!m2t_pixel_loss_make(kind, param, (float)wn[k], &seed[k])) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss: bad kind");
    CK(launch_vgg_tap_partial(xa[l], ws + L.ytap[k], n, value, part + (size_t)k * PART, st));
  }
  CK(launch_vgg_finish(part, nblk, wn, inv_n, accumulate, loss_out, per_tap_out, st));
  if (!gx_add) return 0;

  // backward: g[l] = the gradient at layer l's convolution output, after its ReLU mask
  CK(launch_vgg_tap_seed(xa[12], ws + L.ytap[4], (long long)L.elems(B, 12), seed[4], ws + L.g[12], st));
  for (int l = NL - 1; l >= 1; --l) {
    const int lv = LEVEL[l];
    if (pool_before(l)) {
      CK(launch_vgg_conv(1, ws + L.g[l], v->packed + v->wb[l], ws + L.gp, B, L.h[lv], L.w[lv], COUT[l], CIN[l], nullptr, nullptr, nullptr,
                         value, st));
      CK(launch_vgg_pool_bwd(xa[l - 1], ws + L.gp, ws + L.g[l - 1], B, L.h[lv - 1], L.w[lv - 1], COUT[l - 1], 1, st));
    } else {
      const int k = tap_of(l - 1);
      const bool seeded = k >= 0 && tw[k] != 0.0;
      CK(launch_vgg_conv(1, ws + L.g[l], v->packed + v->wb[l], ws + L.g[l - 1], B, L.h[lv], L.w[lv], COUT[l], CIN[l], nullptr, xa[l - 1],
                         seeded ? ws + L.ytap[k] : nullptr, seeded ? seed[k] : value, st));
    }
  }
  return launch_vgg_first_bwd(ws + L.g[0], (const float*)(v->packed + v->w0), x, gx_add, sx.img, sx.chs, sx.row, R, clamp, B, H, W, st);
}

bool vgg_loaded(const m2t_vgg* v) { return v && v->packed; }
bool vgg_size_supported(int H, int W) { return H >= MIN_SIDE && W >= MIN_SIDE; }

int vgg_check_common(const char* who, const double* tw, double scale, float R, int kind, float param) {
  static thread_local char msg[160];
  auto fail = [&](const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return m2t_set_error(M2T_ERR_ARG, msg); };
  if (!tw) return fail("null tap weights");
  for (int k = 0; k < NTAP; ++k) if (!std::isfinite(tw[k])) return fail("tap weights must be finite");
  if (!std::isfinite(scale)) return fail("scale / weight must be finite");
  if (!(R > 0.f) || !std::isfinite(R)) return fail("the data range must be a finite number > 0");
  M2TPixelLoss t;
  if (!m2t_pixel_loss_make(kind, param, 1.f, &t)) return fail("unknown kind, or eps / beta not finite and > 0");
  return 0;
}

extern "C" int m2t_vgg_loss_tensor(const m2t_vgg* v, const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride,
                                   int x_row_stride, float data_range, int clamp, int kind, float param, const double* tap_weights,
                                   double scale, float* gx_add, float* loss_out, double* per_tap_out, int accumulate, void* workspace,
                                   void* stream) {
  if (!v || !x || !y || !loss_out || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss_tensor: null argument");
  if (B < 1 || B > MAX_B) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss_tensor: need 1 <= B <= 32767");
  if (C != 1 && C != 3) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss_tensor: C must be 1 or 3");
  if (!vgg_size_supported(H, W)) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss_tensor: H and W must be at least 16 (four 2 x 2 pools before relu5_1)");
  CK(vgg_check_common("m2t_vgg_loss_tensor", tap_weights, scale, data_range, kind, param));
  if (x_row_stride < W || x_image_stride % C != 0 || x_image_stride / C < (long long)(H - 1) * x_row_stride + W)
    return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_loss_tensor: strides of x do not hold a [C][H][W] image (channel stride = x_image_stride / C)");
  if (!v->packed) return m2t_set_error(M2T_ERR_STATE, "m2t_vgg_loss_tensor: call m2t_vgg_load_weights first (no VGG19 weights ship with the library)");
  return launch_vgg_loss(v, x, y, B, C, H, W, x_image_stride, x_row_stride, data_range, clamp ? 1 : 0, kind, param, tap_weights, scale,
                         (double)B, gx_add, loss_out, per_tap_out, accumulate ? 1 : 0, workspace, (hipStream_t)stream);
}

// ---- operator entries --------------------------------------------------------------------------------------------------------------
static int op_check(const char* who, const m2t_vgg* v, int layer, const void* a, const void* b, int N, int H, int W) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return m2t_set_error(code, msg); };
  if (!v || !a || !b) return fail(M2T_ERR_ARG, "null argument");
  if (layer < 0 || layer >= NL) return fail(M2T_ERR_ARG, "layer must be 0 .. 12");
  if (N < 1 || N > MAX_B || H < 1 || W < 1 || (long long)H * W > (1LL << 30)) return fail(M2T_ERR_ARG, "bad N, H or W");
  if (!v->packed) return fail(M2T_ERR_STATE, "call m2t_vgg_load_weights first");
  return 0;
}

extern "C" int m2t_vgg_conv_forward(const m2t_vgg* v, int layer, const void* in, void* out, int N, int H, int W, float data_range,
                                    void* stream) {
  CK(op_check("m2t_vgg_conv_forward", v, layer, in, out, N, H, W));
  const float* bias = (const float*)(v->packed + v->bias[layer]);
  if (layer == 0) {
    if (!(data_range > 0.f) || !std::isfinite(data_range)) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_conv_forward: bad data_range");
    return launch_vgg_first_fwd((const float*)in, 3LL * H * W, (long long)H * W, W, data_range, 0, (const float*)(v->packed + v->w0), bias, out,
                                N, H, W, (hipStream_t)stream);
  }
  return launch_vgg_conv(0, in, v->packed + v->wf[layer], out, N, H, W, CIN[layer], COUT[layer], bias, nullptr, nullptr, M2TPixelLoss(),
                         (hipStream_t)stream);
}

extern "C" int m2t_vgg_conv_backward(const m2t_vgg* v, int layer, const void* gout, const void* relu_of, void* gin, int N, int H, int W,
                                     float data_range, void* stream) {
  CK(op_check("m2t_vgg_conv_backward", v, layer, gout, gin, N, H, W));
  if (layer == 0) {
    if (!(data_range > 0.f) || !std::isfinite(data_range)) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_conv_backward: bad data_range");
    return launch_vgg_first_bwd(gout, (const float*)(v->packed + v->w0), (const float*)gin, (float*)gin, 3LL * H * W, (long long)H * W, W,
                                data_range, 0, N, H, W, (hipStream_t)stream);
  }
  return launch_vgg_conv(1, gout, v->packed + v->wb[layer], gin, N, H, W, COUT[layer], CIN[layer], nullptr, relu_of, nullptr, M2TPixelLoss(),
                         (hipStream_t)stream);
}

static int pool_check(const char* who, const void* a, const void* b, int N, int H, int W, int C) {
  static thread_local char msg[160];
  if (!a || !b || N < 1 || N > MAX_B || H < 2 || W < 2 || C < 8 || C % 8 != 0 || (long long)H * W > (1LL << 30)) {
    snprintf(msg, sizeof msg, "%s: null argument, N < 1, H or W < 2, or C not a multiple of 8", who);
    return m2t_set_error(M2T_ERR_ARG, msg);
  }
  return 0;
}
extern "C" int m2t_vgg_pool_forward(const void* in, void* out, int N, int H, int W, int C, void* stream) {
  CK(pool_check("m2t_vgg_pool_forward", in, out, N, H, W, C));
  return launch_vgg_pool_fwd(in, out, N, H, W, C, (hipStream_t)stream);
}
extern "C" int m2t_vgg_pool_backward(const void* a, const void* gout, void* gin, int N, int H, int W, int C, int relu, void* stream) {
  CK(pool_check("m2t_vgg_pool_backward", a, gin, N, H, W, C));
  if (!gout) return m2t_set_error(M2T_ERR_ARG, "m2t_vgg_pool_backward: null gout");
  return launch_vgg_pool_bwd(a, gout, gin, N, H, W, C, relu ? 1 : 0, (hipStream_t)stream);
}
