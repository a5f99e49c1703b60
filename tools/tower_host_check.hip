// tower_host_check.hip -- a stand-alone host program around the C ABI of the two frozen towers (m2t_swin.hip, m2t_text.hip), for a
// sanitizer run of their HOST code on a machine without a device.  The passes index fixed-size handle tables filled at create
// (m2t_tower.h), so an index past the end of a table is what such a run is for:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/tower_host_check.hip m2trans_amd/csrc/m2t_swin.hip \
//         m2trans_amd/csrc/m2t_text.hip m2trans_amd/csrc/k_swin.hip m2trans_amd/csrc/k_swin_bwd.hip m2trans_amd/csrc/k_gemm.hip \
//         -o tower_host_check
//   ./tower_host_check
//
// It links the towers and their launchers from the library's sources; the four hooks they call into m2t_api.hip (the three error
// hooks, the dynamic-LDS opt-in) are defined here.  It creates and destroys Swin handles (max_images 1, 2, 8; both dtypes) and text
// handles (max_seqs 1, 8; max_len 1, 77, 128), walks every param: / numel: / ws: / wsn: key, lays the Swin grad workspace for every
// n_grad from 1 to max_images and back down with the gws: / gwsn: keys after each, and calls every entry's refusals (null
// arguments, no weights, counts out of range).  No valid encode is attempted: that needs a device.  Exit status 0 = every
// expectation held.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <string>
#include <vector>
#include "../include/m2t.h"
#include "../include/m2t_swin.h"
#include "../include/m2t_text.h"
#include "../m2trans_amd/csrc/m2t_kernels.h"

static char g_last[256];
int m2t_set_error_at(int code, const char* who, const char* what) {
  snprintf(g_last, sizeof g_last, "%s: %s", who, what);
  return code;
}
int m2t_set_error(int code, const char* msg) {
  snprintf(g_last, sizeof g_last, "%s", msg);
  return code;
}
int m2t_set_hip_error(hipError_t e, const char* file, int line) {
  snprintf(g_last, sizeof g_last, "%s:%d: %s", file, line, hipGetErrorString(e));
  return (int)e;
}
int m2t_ensure_dynamic_lds(const void* kernel, int bytes) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e == hipSuccess ? 0 : m2t_set_hip_error(e, __FILE__, __LINE__);
}

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      ++failures;                                                           \
      fprintf(stderr, "line %d: expectation failed: %s (last error: %s)\n", __LINE__, #cond, g_last); \
    }                                                                       \
  } while (0)

static const char* const SWIN_WS[] = {"packed", "fbias", "crops", "A0", "X", "Hn", "QKV", "AO", "MH", "emb"};
static const char* const TEXT_WS[] = {"packed", "fbias", "ids", "mask", "X", "XM", "Y", "QKV", "AO", "MH", "pooled"};
static const int DEPTHS[4] = {2, 2, 6, 2};

// every region of the Swin grad workspace, restated from the geometry
static std::vector<std::string> grad_names() {
  std::vector<std::string> v;
  for (int s = 0; s < 4; ++s) {
    for (int j = 0; j < DEPTHS[s]; ++j)
      for (const char* k : {"qkvT", "oT", "fc1T", "fc2T"}) v.push_back("encoder.layers." + std::to_string(s) + ".blocks." + std::to_string(j) + "." + k);
    if (s < 3) v.push_back("encoder.layers." + std::to_string(s) + ".downsample.redT");
  }
  for (const char* k : {"gR", "gF", "gT", "gC", "gQ", "gA", "e0", "xf", "hnf", "MD"}) v.push_back(k);
  for (int s = 0; s < 4; ++s) {
    for (int j = 0; j < DEPTHS[s]; ++j)
      for (const char* k : {"xin", "xmid", "qkv", "gder"}) v.push_back("s" + std::to_string(s) + "b" + std::to_string(j) + "." + k);
    if (s < 3) v.push_back("m" + std::to_string(s));
  }
  return v;
}

// param: / numel: of every tensor (they tile [0, num_params)), ws: / wsn: of every region (inside workspace_bytes), the -1 answers
template <typename H, typename Q, typename N, size_t NWS>
static void walk_inventory(const H* h, Q query, N param_name, const char* const (&ws)[NWS]) {
  const long long nt = query(h, "num_param_tensors"), np = query(h, "num_params"), wb = query(h, "workspace_bytes");
  EXPECT(nt > 0 && np > 0 && wb > 0);
  long long next = 0;
  for (int i = 0; i < nt; ++i) {
    const char* nm = param_name(h, i);
    EXPECT(nm != nullptr);
    if (!nm) break;
    const long long off = query(h, (std::string("param:") + nm).c_str()), cnt = query(h, (std::string("numel:") + nm).c_str());
    EXPECT(off == next && cnt > 0);
    next = off + cnt;
  }
  EXPECT(next == np);
  EXPECT(param_name(h, (int)nt) == nullptr && param_name(h, -1) == nullptr);
  EXPECT(query(h, "param:no.such.parameter") == -1 && query(h, "numel:no.such.parameter") == -1);
  for (const char* nm : ws) {
    const long long off = query(h, (std::string("ws:") + nm).c_str()), cnt = query(h, (std::string("wsn:") + nm).c_str());
    EXPECT(off >= 0 && off % 256 == 0 && cnt > 0 && off < wb);
  }
  EXPECT(query(h, "ws:no_such_tensor") == -1 && query(h, "wsn:no_such_tensor") == -1 && query(h, "packed:pe") == -1);
  EXPECT(query(h, nullptr) == -1);
}

static void check_swin(int max_images, int dt) {
  m2t_swin* h = nullptr;
  EXPECT(m2t_swin_create(&h, max_images, dt) == 0 && h);
  if (!h) return;
  EXPECT(m2t_swin_query(h, "max_images") == max_images);
  walk_inventory(h, m2t_swin_query, m2t_swin_param_name, SWIN_WS);
  const std::vector<std::string> names = grad_names();
  EXPECT(m2t_swin_query(h, "gws:gR") == -1 && m2t_swin_query(h, "gwsn:gR") == -1);      // before the first layout
  EXPECT(m2t_swin_grad_workspace_bytes(h, 0) == M2T_ERR_ARG && m2t_swin_grad_workspace_bytes(h, max_images + 1) == M2T_ERR_ARG);
  EXPECT(m2t_swin_grad_workspace_bytes(nullptr, 1) == M2T_ERR_ARG);
  std::vector<int> counts;
  for (int ng = 1; ng <= max_images; ++ng) counts.push_back(ng);
  for (int ng = max_images - 1; ng >= 1; --ng) counts.push_back(ng);
  for (int ng : counts) {
    const long long nbytes = m2t_swin_grad_workspace_bytes(h, ng);
    EXPECT(nbytes > 0);
    for (const std::string& nm : names) {
      const long long off = m2t_swin_query(h, ("gws:" + nm).c_str()), cnt = m2t_swin_query(h, ("gwsn:" + nm).c_str());
      EXPECT(off >= 0 && off % 256 == 0 && cnt > 0 && off < nbytes);
    }
    EXPECT(m2t_swin_query(h, "gwsn:gR") == (long long)ng * 3136 * 96);
    EXPECT(m2t_swin_query(h, "gws:no_such_tensor") == -1 && m2t_swin_query(h, "gwsn:no_such_tensor") == -1);
  }
  // the refusals: never a launch.  The pointers below are never dereferenced on the host before the checks return
  float* dev = reinterpret_cast<float*>(0x1000);
  void* ws = reinterpret_cast<void*>(0x2000);
  const int crops[3] = {0, 0, 0};
  EXPECT(m2t_swin_load_weights(nullptr, dev, ws, nullptr) == M2T_ERR_ARG && m2t_swin_load_weights(h, nullptr, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_load_weights(h, dev, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode(nullptr, dev, 1, 224, 224, crops, 1, dev, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode(h, nullptr, 1, 224, 224, crops, 1, dev, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode(h, dev, 1, 224, 224, nullptr, 1, dev, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode(h, dev, 1, 224, 224, crops, 1, nullptr, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode(h, dev, 1, 224, 224, crops, 1, dev, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode_pair(h, dev, 1, nullptr, 1, 224, 224, crops, 1, dev, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode_ex(h, dev, 0, nullptr, 0, 224, 224, crops, 1, dev, ws, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode(h, dev, 1, 224, 224, crops, 1, dev, ws, nullptr) == M2T_ERR_STATE);      // no weights loaded
  EXPECT(m2t_swin_encode_grad(nullptr, dev, 1, nullptr, 0, 224, 224, crops, 1, 1, dev, ws, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode_grad(h, dev, 1, nullptr, 0, 224, 224, crops, 1, 1, dev, ws, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode_grad(h, dev, 1, nullptr, 0, 224, 224, crops, 1, 2, dev, ws, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_encode_grad(h, dev, 1, nullptr, 0, 224, 224, crops, 1, 1, dev, ws, ws, nullptr) == M2T_ERR_STATE);
  EXPECT(m2t_swin_backward(nullptr, dev, 1, dev, ws, ws, nullptr) == M2T_ERR_ARG && m2t_swin_backward(h, nullptr, 1, dev, ws, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_backward(h, dev, 1, nullptr, ws, ws, nullptr) == M2T_ERR_ARG && m2t_swin_backward(h, dev, 1, dev, nullptr, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_backward_ex(h, dev, 1, dev, ws, nullptr, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_swin_backward(h, dev, 1, dev, ws, ws, nullptr) == M2T_ERR_STATE);                    // no weights, no stash
  m2t_swin_destroy(h);
}

static void check_text(int max_seqs, int max_len, int dt) {
  m2t_text* h = nullptr;
  EXPECT(m2t_text_create(&h, max_seqs, max_len, dt) == 0 && h);
  if (!h) return;
  EXPECT(m2t_text_query(h, "max_seqs") == max_seqs && m2t_text_query(h, "max_len") == max_len && m2t_text_query(h, "max_images") == -1);
  walk_inventory(h, m2t_text_query, m2t_text_param_name, TEXT_WS);
  float* dev = reinterpret_cast<float*>(0x1000);
  void* ws = reinterpret_cast<void*>(0x2000);
  const int ids[1] = {0}, mask[1] = {1};
  EXPECT(m2t_text_load_weights(nullptr, dev, ws, nullptr) == M2T_ERR_ARG && m2t_text_load_weights(h, nullptr, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_text_load_weights(h, dev, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_text_encode(nullptr, ids, mask, 1, 1, dev, ws, nullptr) == M2T_ERR_ARG && m2t_text_encode(h, nullptr, mask, 1, 1, dev, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_text_encode(h, ids, nullptr, 1, 1, dev, ws, nullptr) == M2T_ERR_ARG && m2t_text_encode(h, ids, mask, 1, 1, nullptr, ws, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_text_encode_ex(h, ids, mask, 1, 1, dev, nullptr, nullptr, nullptr) == M2T_ERR_ARG);
  EXPECT(m2t_text_encode(h, ids, mask, 1, 1, dev, ws, nullptr) == M2T_ERR_STATE);                 // no weights loaded
  m2t_text_destroy(h);
}

int main() {
  m2t_swin* hs = nullptr;
  m2t_text* ht = nullptr;
  EXPECT(m2t_swin_create(nullptr, 1, M2T_F32) == M2T_ERR_ARG && m2t_swin_create(&hs, 0, M2T_F32) == M2T_ERR_ARG && m2t_swin_create(&hs, 1, 7) == M2T_ERR_ARG);
  EXPECT(m2t_text_create(nullptr, 1, 1, M2T_F32) == M2T_ERR_ARG && m2t_text_create(&ht, 0, 1, M2T_F32) == M2T_ERR_ARG);
  EXPECT(m2t_text_create(&ht, 1, 129, M2T_F32) == M2T_ERR_ARG && m2t_text_create(&ht, 1, 1, 7) == M2T_ERR_ARG);
  EXPECT(m2t_swin_query(nullptr, "max_images") == -1 && m2t_text_query(nullptr, "max_len") == -1);
  EXPECT(m2t_swin_param_name(nullptr, 0) == nullptr && m2t_text_param_name(nullptr, 0) == nullptr);
  m2t_swin_destroy(nullptr);
  m2t_text_destroy(nullptr);
  for (int dt : {M2T_F32, M2T_BF16}) {
    for (int max_images : {1, 2, 8}) check_swin(max_images, dt);
    for (int max_seqs : {1, 8})
      for (int max_len : {1, 77, 128}) check_text(max_seqs, max_len, dt);
  }
  if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
  printf("tower_host_check: ok\n");
  return 0;
}
