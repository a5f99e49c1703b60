// m2t_api.hip -- the C ABI (include/m2t.h): plan, whole-model forward / backward launch
// sequences, optimiser and the stand-alone operators.  Host code only; every kernel lives in
// the k_*.hip files.  The launch sequence restates M2Trans.forward / CFTM.forward
// (models/M2Trans_network.py:58-76,132-164) and train.py:199-210.
#include <cstring>
#include <cstdio>
#include "m2t_plan_layout.h"
#include "../../include/m2t_spectral.h"
#include "../../include/m2t_msssim.h"
#include "../../include/m2t_vif.h"
#include "../../include/m2t_gmsd.h"
#include "../../include/m2t_wavelet.h"
#include "../../include/m2t_consistency.h"
#include "../../include/m2t_perceptual.h"

static thread_local std::string g_err;
int m2t_set_hip_error(hipError_t e, const char* file, int line) {
  char buf[512];
  snprintf(buf, sizeof(buf), "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
  g_err = buf;
  return (int)e;
}
int m2t_set_error(int code, const char* msg) { g_err = msg; return code; }
int m2t_set_error_at(int code, const char* who, const char* what) { g_err = std::string(who) + ": " + what; return code; }

int m2t_ensure_dynamic_lds(const void* kernel, int bytes) {
  static thread_local std::map<std::pair<int, const void*>, int> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  auto it = done.find({dev, kernel});
  if (it != done.end() && it->second >= bytes) return 0;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  done[{dev, kernel}] = bytes;
  return 0;
}

// The plan: its shape and the options that decide the layout (m2t_plan_geom, m2t_plan_layout.h), then everything else.
// hd's parameter and pack offsets are set once by m2t_plan_create; lay.ws, hd's workspace offsets and the health rows are rebuilt
// by resolve_layout() from the one region table, for the mode in force, after every change of an option: nothing is kept aside
struct m2t_plan : m2t_plan_geom {
  m2t_layout lay;                    // names -> offsets: read at creation and by m2t_plan_query only
  m2t_plan_handles hd;
  m2t_sched sc;                      // resolve_schedule() after every change of an option
  m2t_health_table ht;               // option "health": the rows of the record, empty on every other plan
  std::vector<m2t_pack_desc> descs;
  std::vector<char> desc_is_qkv;             // per descriptor: a packed form of a qkv_conv.weight
  std::vector<int> pack_blocks;              // (descriptor, chunk) pairs: one workgroup of the packing kernel each.  Order: every
                                             // descriptor that is always needed, then the plain copies of the C >= 64 qkv weights (read only by the
                                             // unfused forward GEMM), then their transposes (read only by the unfused data-gradient GEMM)
  int pack_nb_base = 0, pack_nb_copy = 0, pack_nb_tr = 0;   // workgroups of the three groups (round 5: the default bf16 path skips the last two:
                                             // 6.3 M of the 14.2 M packed elements, the transposes being the slowest gathers of the kernel)
  bool have_seed = false, have_acts = false;
  int health_on = 1;                   // option "health_on": the record of a plan with "health" > 0 is taken (1) or skipped (0)
  bool ws_initialised = false;         // m2t_plan_init_workspace has run: "inference" is frozen, and so is every option of an inference plan
  // m2t_l1_loss_deferred: the loss and the seed are produced inside the next m2t_backward (round 5)
  bool l1_deferred = false;
  const float* l1_hr = nullptr; float* l1_loss_out = nullptr; float l1_sc = 0.f, l1_R = 0.f;
  M2TPixelLoss l1_pl;                  // the deferred loss's kind and factors (m2t_pixel_loss_deferred; m2t_l1_loss_deferred: l1)
  // ---- raw option values (m2t_set_option; include/m2t.h documents each).  Only resolve_schedule combines them. ----
  int use_fp32_fast = 1;               // fp32: the v_mfma_f32_32x32x2_f32 GEMM / qkv weight-gradient kernels of round 5 (k_gemm.hip); 0 = the 16x16x4 kernels
  int use_fused_l1 = 1;                // bf16 x4: the clamp + L1 seed inside the fused tail backward when the loss was requested through m2t_l1_loss_deferred
  int use_tail_bwd32 = 1;              // bf16 x4, recomputing fused tail backward: the 32x32x16-MFMA kernel of round 6 (k_tail_bwd.hip); 0 = the 16x16x32 kernel
  bool use_side = true;
  bool debug_skip_side = false;        // timing experiments only: skip every parameter-gradient kernel (results are WRONG)
  bool use_fused_tail_bwd = true;      // x4 bf16: k_tail_bwd.hip instead of four HR kernels                              } option "fused_tail":
  bool use_fused_tail_fwd = true;      // x4 bf16: tail.3 expansion + GELU + tail conv in one kernel, gelu(t2) / gelu'(t2) never stored } 0 / 1 / 2 / 3
  bool use_stream_tail_fwd = true;     // ... as the row-streaming kernel (k_tail_stream.hip, round 4: 152 vs 229 us, same bits); 2 = the 16x16-tile kernel
  bool use_stream_tail_bwd = false;    // x4: the row-streaming BACKWARD (k_tail_bwd_stream.hip) instead of the tile kernel: option value 4, kept for
                                       // A/B -- same data gradient bits, 580 against 377 us stand-alone at batch 16
                                       // (with bf16 mode's exp2 / rcp GELU: 5.30 vs 5.34 ms per step and 1.6 GB less HBM traffic;
                                       // with the erf form of round 2 it was 1 % slower)
                                       // x2 / x3, bf16, "fused_tail" >= 1: expansion + PixelShuffle + GELU + tail conv as ONE row-streaming forward kernel and
                                       // ONE recomputing backward kernel (k_tail_stream.hip, k_tail_bwd_stream.hip): gelu(t) / gelu'(t) are never stored
  int use_fused_prep_bwd = 1;          // bf16: branch_prep_bwd of branch 4 inside the attention backward of branch 3 (round 4)
  int use_fused_prep_fwd = 1;          // bf16 C = 64 / 256 branches: branch_prep inside the fused forward attention kernel (round 4)
  int fused_attn_fwd2 = 0;             // bf16 C = 256 forward branch with branch_prep inside: the two-windows-per-CU kernels (k_attn_fwd2.hip, round 5):
                                       // 0 = never (default: measured equal to the one-window kernel within 2 %, profiles/README.md), 1 = 4-wave workgroups
                                       // (two per CU), 2 = 8-wave workgroups of two windows, -1 = variant 1 when the branch has more windows than CUs (256)
  int use_fused_norm_red = 0;          // bf16 with the C = 16 prep kernel: the first stage of the InstanceNorm backward reduction rides in that launch (round 5;
                                       // measured SLOWER, -2.2 % on the step: both roles are memory-heavy, profiles/README.md -- kept for A/B)
  int fork_on_kernel = 1;              // a fork event rides on the dispatch it follows (its stop event) instead of a marker packet behind it:
                                       // same-box A/B 4.757 -> 4.726 ms (config 1), 8.536 -> 8.469 (config 3); not under stream capture
  int gate_branch = -1;                // side-stream gate: -1 ungated (a branch's side work follows its attention launch), else the branch (3..0)
                                       // behind whose attention launch a block's parameter-gradient work is released.  Same-box A/B (config 1),
                                       // end of round 3 (one buffer-set wait per block instead of one per branch): ungated 4.84 ms, 2 = 4.95,
                                       // 0 = 5.10, 3 = 5.10, 1 = 5.14, one stream 5.35; batch 32: ungated 8.78, 2 = 8.76.  (While the main chain
                                       // still waited for the side stream once per BRANCH the gate paid: round 2: 1 = 5.49, 2 = 5.60, ungated 5.64)
  bool use_resident_attn_bwd = true;   // bf16: whole-window-resident attention backward (k_attn_res.hip)         } option "attn_bwd":
  bool use_fused_conv_bwd = true;      // bf16 conv3x3 64 -> 64 backward: data + weight / bias gradient in one row-streaming pass (k_conv.hip)
  int use_conv_rows = 1;               // bf16 conv3x3 64 -> 64: row-streaming LDS-DMA kernel (k_conv.hip); 0 = the tile kernel
  int wgrad_big_tiles = -1;            // C = 256 qkv weight gradient: 128 x 128 output tiles (k_gemm.hip); value = target workgroups,
                                       // 0 = off, -1 = auto: 256 from 24 576 rows on (batch 32: 9.82 vs 9.93 ms; batch 16: 5.53 vs 5.49)
  bool use_fused_qkv_dgrad = true;     // bf16, C = 64 / 256: projection data gradient inside that kernel                } 0 .. 3
  bool use_c16_prep = true;            // bf16, C = 16: overlap-add + projection data gradient + branch_prep_bwd in one kernel }
  int use_fused_c16_fwd = 2;           // bf16, C = 16 branch: norm apply + qkv projection + attention + residual in one kernel (k_attn_c16.hip);
                                       // 2: ... and qkv1 is not stored: the wave-per-window backward recomputes it from d1 (needs attn_bwd >= 1)
  int use_fused_attn_fwd = 2;          // bf16, C = 64 / 256: qkv projection + attention + epilogue in one kernel (k_attn_fused.hip);
                                       // 2: ... and qkv2 (C = 64) is not stored: the resident backward recomputes it from d2 (needs attn_bwd = 2)
  // deferred, batched parameter-gradient reductions (m2t_backward): slabs live in the "arena" workspace
  // region; the descriptor table is identical every step, so it is uploaded once
  std::vector<m2t_red_desc> red_descs;
  bool red_uploaded = false;
  // m2t_backward_ex with some stages frozen: such a pass never publishes or checks the table above; it reduces everything once at
  // its end through a table of its own stage mask, uploaded on the first pass with that mask into a plan-owned device buffer
  struct MaskTable { std::vector<m2t_red_desc> descs; void* dev = nullptr; bool uploaded = false; };
  std::map<std::vector<unsigned char>, MaskTable> mask_tables;
  hipStream_t side = nullptr;
  // gradient buckets: [lo, hi) float ranges of the flat gradient buffer in the order m2t_backward completes them
  // (tail, block pairs from the last to the first, head); one event each, recorded behind the bucket's reduction
  std::vector<std::pair<long long, long long>> buckets;
  std::vector<hipEvent_t> bucket_events;
  std::vector<hipEvent_t> events;
  int ensure_side(hipStream_t caller) {
    if (side) return 0;
    // (a CU-masked side stream and a side stream of LOWER priority than the caller's were both measured and are slower: profiles/README.md,
    //  round 2.)  The side stream takes the CALLER'S priority: a caller that runs the step on a high-priority stream beside other work of
    //  its own (the MedCLIP encoder of configs[2] on a normal-priority stream, round 5) gets both halves of the backward pass ahead of it
    int prio = 0;
    if (hipStreamGetPriority(caller, &prio) != hipSuccess) prio = 0;
    if (hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio) != hipSuccess) return -1;
    events.resize(192);
    for (auto& e : events)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return -1;
    bucket_events.resize(buckets.size());
    for (auto& e : bucket_events)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return -1;
    return 0;
  }
  ~m2t_plan() {
    for (auto e : events) if (e) (void)hipEventDestroy(e);
    for (auto e : bucket_events) if (e) (void)hipEventDestroy(e);
    // the caller releases the workspace right after this: nothing of the plan's own stream may still be running in it
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    for (auto& kv : mask_tables) if (kv.second.dev) (void)hipFree(kv.second.dev);
  }

  long long add_pack(const std::string& n, const std::string& src, int kind, long long cnt, int d0, int d1, int d2) {
    m2t_pack_desc d;
    d.src_off = lay.poff.at(src); d.dst_off = lay.add_pack(n, cnt); d.n = cnt; d.kind = kind; d.d0 = d0; d.d1 = d1; d.d2 = d2;
    descs.push_back(d);
    desc_is_qkv.push_back(src.find("qkv_conv.weight") != std::string::npos ? 1 : 0);
    return d.dst_off;
  }
};

static void resolve_schedule(m2t_plan* p) {
  const bool bf = p->dt != M2T_F32, x4 = p->scale == 4;
  m2t_sched& s = p->sc;
  s.resident_bwd = bf && p->use_resident_attn_bwd;
  s.fused_dgrad = s.resident_bwd && p->use_fused_qkv_dgrad;
  s.c16_prep = s.fused_dgrad && p->use_c16_prep;
  s.prep_in_bwd = s.fused_dgrad && p->use_fused_prep_bwd;          // (branches 3 and 4 share a level and a window grid)
  s.norm_red_in_prep = s.c16_prep && p->use_fused_norm_red;
  s.c16_fused_fwd = bf && p->use_fused_c16_fwd != 0;
  s.c16_recompute = s.resident_bwd && p->use_fused_c16_fwd == 2;
  s.c64_fused_fwd = bf && p->use_fused_attn_fwd != 0;
  s.prep_in_fwd = s.c64_fused_fwd && p->use_fused_prep_fwd;
  s.c64_recompute = s.fused_dgrad && p->use_fused_attn_fwd == 2;
  s.fwd2 = 0;
  if (s.prep_in_fwd) {
    // the C = 256 branches run at H / 4 x W / 4 in 8 x 8 windows.  -1: only with more windows than CUs; variant 2 pairs windows
    const long long nwin = (long long)p->B * (p->H / 32) * (p->W / 32);
    const bool even = (((p->H / 32) * (p->W / 32)) & 1) == 0;
    if (p->fused_attn_fwd2 != 0 && !(p->fused_attn_fwd2 < 0 && nwin <= 256)) s.fwd2 = (p->fused_attn_fwd2 == 2 && even) ? 2 : 1;
  }
  const bool fused_tail = bf && p->use_fused_tail_bwd;             // "fused_tail" >= 1
  if (!x4) {
    s.tail_fwd = fused_tail ? TAIL_FWD_X23_STREAM : TAIL_FWD_PLAIN;
    s.tail_bwd = fused_tail ? TAIL_BWD_X23_STREAM : TAIL_BWD_PLAIN;
  } else {
    const bool rc = fused_tail && p->use_fused_tail_fwd;           // gelu(t2) / gelu'(t2) are not stored: the backward recomputes them
    s.tail_fwd = !rc ? TAIL_FWD_PLAIN : (p->use_stream_tail_fwd ? TAIL_FWD_STREAM : TAIL_FWD_TILE);
    s.tail_bwd = !fused_tail ? TAIL_BWD_PLAIN : !rc ? TAIL_BWD_STORED : p->use_stream_tail_bwd ? TAIL_BWD_STREAM
                 : (p->use_tail_bwd32 ? TAIL_BWD_RC32 : TAIL_BWD_RC16);
  }
  s.l1_in_tail = p->use_fused_l1 && (s.tail_bwd == TAIL_BWD_RC16 || s.tail_bwd == TAIL_BWD_RC32);
  s.conv_rows = bf && p->use_conv_rows;
  s.conv_variant = p->use_conv_rows ? 0 : 1;
  s.fused_conv_bwd = bf && p->use_fused_conv_bwd && conv3x3_c64_bwd_fusable(p->B, p->H, p->W);
  s.need_copy = !s.c64_fused_fwd;
  s.need_tr = !s.fused_dgrad;
  s.stores_qkv1 = !s.c16_recompute;
  s.stores_qkv2 = !s.c64_recompute;
  s.stores_t1 = s.tail_fwd != TAIL_FWD_X23_STREAM;
  s.stores_t2 = x4 && s.tail_fwd == TAIL_FWD_PLAIN;
  s.fork_on_kernel = p->use_side && p->fork_on_kernel;
}

static int health_record(m2t_plan* p, int phase, const void* ext, char* ws, hipStream_t st) {
  const m2t_plan_handles& hd = p->hd;
  const int row0 = phase ? p->ht.rows_fwd : 0, item0 = phase ? p->ht.items_fwd : 0;
  const int nrows = phase ? (int)p->ht.descs.size() - row0 : p->ht.rows_fwd;
  const int nitems = phase ? (int)(p->ht.work.size() / 2) - item0 : p->ht.items_fwd;
  return launch_health_record(ws, ext, (const m2t_health_desc*)(ws + hd.health_descs), (const int*)(ws + hd.health_work),
                              (double*)(ws + hd.health_part), (double*)(ws + hd.health), phase, row0, nrows, item0, nitems, st);
}

// the name table, the workspace handles and the health rows that go with the mode and the schedule in force (resolve_schedule first)
static void resolve_layout(m2t_plan* p) { m2t_resolve_workspace(*p, p->sc, p->hd, p->lay.ws, p->ht); }
static int refuse_inference(const m2t_plan* p, const char* who) {
  if (!p->inference) return 0;
  return m2t_set_error_at(M2T_ERR_STATE, who, "this is an inference plan (option \"inference\"): it keeps no activations and no seed");
}

extern "C" int m2t_version(void) { return 100; }
extern "C" const char* m2t_last_error_string(void) { return g_err.c_str(); }

extern "C" int m2t_plan_create(m2t_plan** out, int B, int H0, int W0, int scale, int n_blocks, int dtype) {
  if (!out || B < 1 || H0 < 2 || W0 < 2 || (scale != 2 && scale != 3 && scale != 4) || n_blocks < 1 ||
      (dtype != M2T_F32 && dtype != M2T_BF16))
    return m2t_set_error(M2T_ERR_ARG, "m2t_plan_create: bad argument");
  m2t_plan* p = new m2t_plan();
  p->B = B; p->H0 = H0; p->W0 = W0; p->scale = scale; p->nb = n_blocks; p->dt = dtype;
  p->esz = p->lay.esz = (dtype == M2T_F32) ? 4 : 2;
  p->H = (H0 + 31) / 32 * 32;
  p->W = (W0 + 31) / 32 * 32;
  if (p->H - H0 >= H0 || p->W - W0 >= W0) { delete p; return m2t_set_error(M2T_ERR_ARG, "m2t_plan_create: reflect pad needs pad < size"); }
  p->P = (long long)p->H * p->W;
  p->Hs = H0 * scale; p->Ws = W0 * scale; p->Hsp = p->H * scale; p->Wsp = p->W * scale;
  const int s = scale;
  m2t_layout& lay = p->lay;
  m2t_plan_handles& hd = p->hd;
  hd = m2t_plan_handles{};
  hd.blk.assign(n_blocks, m2t_block_handles{});
  auto param = [&](const std::string& n, long long cnt) { lay.add_param(n, cnt); return lay.poff[n]; };
  // ---- parameters: trainable tensors in the reference's registration order ----
  hd.head_w = param("head.weight", 64 * 3 * 9);
  hd.head_b = param("head.bias", 64);
  for (int b = 0; b < n_blocks; ++b) {
    m2t_block_handles& bh = hd.blk[b];
    for (int i = 0; i < 4; ++i) {
      const int C = BR_C[i];
      const std::string pre = "body." + std::to_string(b) + ".attn" + std::to_string(i + 1) + ".";
      bh.rel_h[i] = param(pre + "rel_h", 10 * C / 2);
      bh.rel_w[i] = param(pre + "rel_w", 10 * C / 2);
      bh.wqkv[i] = param(pre + "qkv_conv.weight", 3LL * C * C);
    }
    const std::string pre = "body." + std::to_string(b) + ".feed_forward.0.";
    bh.ffw = param(pre + "weight", 64 * 64 * 9);
    bh.ffb = param(pre + "bias", 64);
  }
  if (s == 4) {
    hd.tail0_w = param("tail.0.weight", 256 * 64); hd.tail0_b = param("tail.0.bias", 256);
    hd.tail3_w = param("tail.3.weight", 256 * 64); hd.tail3_b = param("tail.3.bias", 256);
    hd.wlast = param("tail.6.weight", 3 * 64 * 9);
  } else {
    hd.tail0_w = param("tail.0.weight", 64LL * s * s * 64); hd.tail0_b = param("tail.0.bias", 64 * s * s);
    hd.wlast = param("tail.3.weight", 3 * 64 * 9);
  }
  // ---- packed weights (element type T) ----
  for (int b = 0; b < n_blocks; ++b) {
    m2t_block_handles& bh = hd.blk[b];
    for (int i = 0; i < 4; ++i) {
      const int C = BR_C[i];
      const std::string src = "body." + std::to_string(b) + ".attn" + std::to_string(i + 1) + ".qkv_conv.weight";
      const std::string k = "b" + std::to_string(b) + ".w" + std::to_string(i + 1);
      bh.w[i] = p->add_pack(k, src, M2T_PACK_COPY, 3LL * C * C, 0, 0, 0);
      bh.wT[i] = p->add_pack(k + "T", src, M2T_PACK_TRANSPOSE, 3LL * C * C, 3 * C, C, 0);
      bh.wF[i] = bh.wTF[i] = -1;
      if (C >= 64) bh.wF[i] = p->add_pack(k + "F", src, M2T_PACK_FRAG16, 3LL * C * C, 3 * C, C, 0);   // k_attn_fused.hip
      if (C >= 64) bh.wTF[i] = p->add_pack(k + "TF", src, M2T_PACK_FRAG16_T, 3LL * C * C, C, 3 * C, 0);  // Wqkv^T fragments: fused data gradient (k_attn_res.hip)
    }
    const std::string src = "body." + std::to_string(b) + ".feed_forward.0.weight";
    const std::string k = "b" + std::to_string(b) + ".";
    bh.wf = p->add_pack(k + "wf", src, M2T_PACK_CONV3, 64 * 64 * 9, 64, 64, 0);
    bh.wfT = p->add_pack(k + "wfT", src, M2T_PACK_CONV3_T, 64 * 64 * 9, 64, 64, 0);
    bh.wfR = p->add_pack(k + "wfR", src, M2T_PACK_CONV3_ROWS, 64 * 64 * 9, 64, 64, 0);      // conv3x3_c64_rows_kernel (bf16)
    bh.wfTR = p->add_pack(k + "wfTR", src, M2T_PACK_CONV3_ROWS_T, 64 * 64 * 9, 64, 64, 0);
  }
  const int r0 = (s == 4) ? 2 : s;
  hd.t0 = p->add_pack("t0", "tail.0.weight", M2T_PACK_SHUF_ROWS, 64LL * r0 * r0 * 64, 64, r0 * r0, 64);
  hd.t0T = p->add_pack("t0T", "tail.0.weight", M2T_PACK_SHUF_ROWS_T, 64LL * r0 * r0 * 64, 64, r0 * r0, 64);
  if (s == 4) {
    hd.t3 = p->add_pack("t3", "tail.3.weight", M2T_PACK_SHUF_ROWS, 256 * 64, 64, 4, 64);
    hd.t3T = p->add_pack("t3T", "tail.3.weight", M2T_PACK_SHUF_ROWS_T, 256 * 64, 64, 4, 64);
  }
  // ---- the sizes the workspace takes from here (m2t_plan_geom): the pack tables, the ring buffer, the slab arena ----
  for (int group = 0; group < 3; ++group) {
    int nb_g = 0;
    for (size_t i = 0; i < p->descs.size(); ++i) {
      const bool big = p->descs[i].n >= 3LL * 64 * 64 && (p->descs[i].kind == M2T_PACK_COPY || p->descs[i].kind == M2T_PACK_TRANSPOSE) && p->desc_is_qkv[i];
      const int gi = !big ? 0 : (p->descs[i].kind == M2T_PACK_COPY ? 1 : 2);
      if (gi != group) continue;
      for (long long c = 0; c * M2T_PACK_CHUNK < p->descs[i].n; ++c) { p->pack_blocks.push_back((int)i); p->pack_blocks.push_back((int)c); ++nb_g; }
    }
    (group == 0 ? p->pack_nb_base : (group == 1 ? p->pack_nb_copy : p->pack_nb_tr)) = nb_g;
  }
  p->n_pack_descs = p->descs.size();
  p->n_pack_block_ints = p->pack_blocks.size();
  p->npacked = (size_t)lay.npacked;
  p->nparams = (size_t)lay.nparams;
  p->vring_elems = window_attn_fwd2_vring_elems(B, p->H / 4, p->W / 4);
  {
    // arena: every slab set of one backward pass (see m2t_backward); sized from the launchers' slab rules
    size_t per_block = (size_t)256 * 9 * 64 * 64 + (size_t)256 * 64;                 // conv wgrad + ff bias partials
    per_block += (size_t)1024 * 768 + (size_t)512 * 12288 + 2 * (size_t)32 * 196608; // qkv wgrads (upper bounds)
    per_block += 4 * (size_t)32 * 2560;                                               // rel-pos partials
    size_t tail = 2 * (size_t)256 * (16384 + 36864) + (size_t)1024 * 2048 + 4 * (size_t)256 * 768 + (size_t)256 * 1728 * 2;
    p->arena_floats = per_block * n_blocks + tail + (size_t)512 * (64 * 32 + 64) + (1u << 20);
  }
  {
    // gradient buckets in completion order (see m2t_backward): the tail, then the blocks in the groups the
    // deferred reductions are flushed in (after every even block index, walking from the last block to the first),
    // then whatever precedes the lowest flushed block (the head).  state_dict order makes each a contiguous range.
    long long hi = lay.nparams;
    p->buckets.push_back({hd.tail0_w, hi});
    hi = hd.tail0_w;
    for (int b = n_blocks - 1; b >= 0; --b)
      if ((b & 1) == 0) {
        p->buckets.push_back({hd.blk[b].rel_h[0], hi});
        hi = hd.blk[b].rel_h[0];
      }
    p->buckets.push_back({0, hi});
  }
  resolve_schedule(p);
  resolve_layout(p);
  *out = p;
  return 0;
}
extern "C" void m2t_plan_destroy(m2t_plan* p) { delete p; }

extern "C" long long m2t_plan_query(const m2t_plan* p, const char* key) {
  if (!p || !key) return -1;
  const std::string k(key);
  const m2t_sched& s = p->sc;
  const bool bf = p->dt != M2T_F32;
  if (k == "padded_h") return p->H;
  if (k == "padded_w") return p->W;
  if (k == "grad_buckets") return (long long)p->buckets.size();
  if (k.rfind("grad_bucket_lo:", 0) == 0) { const size_t i = (size_t)atoll(k.c_str() + 15); return i < p->buckets.size() ? p->buckets[i].first : -1; }
  if (k.rfind("grad_bucket_hi:", 0) == 0) { const size_t i = (size_t)atoll(k.c_str() + 15); return i < p->buckets.size() ? p->buckets[i].second : -1; }
  if (k.rfind("opt:", 0) == 0) {        // the options IN FORCE (profile.py prices the kernels that actually run): an option whose
    const std::string o = k.substr(4);  // precondition is off did not run
    if (o == "side_stream") return p->use_side;
    if (o == "fork_on_kernel") return s.fork_on_kernel;
    if (o == "fp32_fast") return !bf && p->use_fp32_fast;
    if (o == "tail_bwd_mfma32") return s.tail_bwd == TAIL_BWD_RC32;
    if (o == "fused_l1") return s.l1_in_tail;
    if (o == "fused_attn_fwd2") return s.fwd2;
    if (o == "fused_norm_red") return s.norm_red_in_prep;
    if (o == "fused_prep_fwd") return s.prep_in_fwd;
    if (o == "fused_prep_bwd") return s.prep_in_bwd;
    if (o == "gate_branch") return p->gate_branch + 1000;      // (offset: -1 is the "unknown key" value of this function)
    if (o == "wgrad_big_tiles") return p->wgrad_big_tiles + 1000;
    if (o == "fused_tail") {
      if (s.tail_bwd == TAIL_BWD_X23_STREAM) return 3;           // x2 / x3: the row-streaming pair or the plain kernels
      if (s.tail_bwd == TAIL_BWD_STREAM) return 4;
      return s.tail_fwd == TAIL_FWD_STREAM ? 3 : (s.tail_fwd == TAIL_FWD_TILE ? 2 : (s.tail_bwd == TAIL_BWD_STORED ? 1 : 0));
    }
    if (o == "attn_bwd") return s.c16_prep ? 3 : (s.fused_dgrad ? 2 : (s.resident_bwd ? 1 : 0));
    if (o == "conv_rows") return s.conv_rows;
    if (o == "fused_conv_bwd") return s.fused_conv_bwd;
    if (o == "fused_attn_fwd") return s.c64_recompute ? 2 : (s.c64_fused_fwd ? 1 : 0);
    if (o == "fused_c16_fwd") return !s.c16_fused_fwd ? 0 : (s.c16_recompute ? 2 : 1);
    if (o == "fused_qkv_dgrad") return s.fused_dgrad;
    if (o == "debug_skip_side") return p->debug_skip_side;
    if (o == "inference") return p->inference;
    if (o == "local_norm") return p->local_norm;
    if (o == "health") return p->health;
    if (o == "health_on") return p->health > 0 && p->health_on;
    return -1;
  }
  // the health record's rows (option "health"): names are resolved here, never by a pass
  if (k.rfind("health_", 0) == 0) {
    const long long rows = p->health > 0 ? (long long)p->ht.descs.size() : 0;
    if (k == "health_rows") return rows;
    if (k.rfind("health_row:", 0) == 0) {
      const std::string name = k.substr(11);
      for (long long r = 0; r < rows; ++r) if (p->ht.names[r] == name) return r;
      return -1;
    }
    if (k.rfind("health_phase:", 0) == 0 || k.rfind("health_name:", 0) == 0) {
      const char* arg = k.c_str() + k.find(':') + 1;
      char* end = nullptr;
      const long long r = strtoll(arg, &end, 10);
      if (end == arg || *end || r < 0 || r >= rows) return -1;
      if (k[7] == 'p') return p->ht.descs[r].phase;
      g_err = p->ht.names[r];                  // "health_name:<index>": the name goes where m2t_last_error_string() reads
      return (long long)p->ht.names[r].size();
    }
    return -1;
  }
  // which stored tensors the current options leave unwritten (tests read the workspace by name)
  if (k == "stores_qkv2") return s.stores_qkv2;
  if (k == "stores_qkv1") return s.stores_qkv1;
  if (k == "stores_t1") return s.stores_t1;
  if (k == "stores_t2") return s.stores_t2;
  return p->lay.query(k, m2t_layout::Q_WS | m2t_layout::Q_WSN | m2t_layout::Q_PACKED);
}

extern "C" int m2t_plan_init_workspace(m2t_plan* p, void* workspace, void* stream) {
  if (!p || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_plan_init_workspace: null");
  char* const ws = (char*)workspace;
  hipError_t e = hipMemcpyAsync(ws + p->hd.pack_descs, p->descs.data(), p->descs.size() * sizeof(m2t_pack_desc),
                                hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  e = hipMemcpyAsync(ws + p->hd.pack_blocks, p->pack_blocks.data(), p->pack_blocks.size() * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  e = hipMemsetAsync(ws + p->hd.zero_page, 0, 256, (hipStream_t)stream);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  std::vector<float> norm_id;                        // (alive until the synchronisation below)
  if (p->hd.norm_id != M2T_NO_REGION) {
    norm_id.assign((size_t)p->B * 64 * 2, 0.f);
    std::fill(norm_id.begin() + (size_t)p->B * 64, norm_id.end(), 1.f);
    e = hipMemcpyAsync(ws + p->hd.norm_id, norm_id.data(), norm_id.size() * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  }
  std::vector<double> health_head;                   // (alive until the synchronisation below)
  if (p->health > 0 && p->hd.health != M2T_NO_REGION) {
    // the record: descriptor table and work list next to the other tables, every row zero, the header row "nothing recorded"
    const size_t rows = p->ht.descs.size();
    e = hipMemcpyAsync(ws + p->hd.health_descs, p->ht.descs.data(), rows * sizeof(m2t_health_desc), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
    e = hipMemcpyAsync(ws + p->hd.health_work, p->ht.work.data(), p->ht.work.size() * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
    e = hipMemsetAsync(ws + p->hd.health, 0, (1 + rows) * health_tile::SLOTS * sizeof(double), (hipStream_t)stream);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
    health_head.assign(health_tile::SLOTS, 0.0);
    health_head[2] = health_head[3] = -1.0;
    health_head[4] = (double)rows;
    e = hipMemcpyAsync(ws + p->hd.health, health_head.data(), health_head.size() * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  }
  e = hipStreamSynchronize((hipStream_t)stream);   // the host table may be freed/moved afterwards
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  p->have_acts = p->have_seed = false;
  p->l1_deferred = false;
  p->ws_initialised = true;
  // red_descs lives in the workspace: a workspace that was just (re)initialised -- possibly another buffer, possibly overwritten --
  // does not hold the published table, so the next all-stages backward publishes it again (the first_backward schedule)
  p->red_uploaded = false;
  return 0;
}

// option "fp32_fast" for the duration of a pass: the thread-local switch the fp32 launchers of k_gemm.hip read, back to its
// default on every exit path
struct F32FastGuard {
  explicit F32FastGuard(int v) { g_m2t_f32_fast = v; }
  ~F32FastGuard() { g_m2t_f32_fast = 1; }
};

extern "C" int m2t_forward(m2t_plan* p, const float* params, const float* x, float* sr, float rgb_range,
                           int keep_activations, void* workspace, void* stream) {
  if (!p || !params || !x || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_forward: null argument");
  if (p->inference && keep_activations != 0)
    return m2t_set_error(M2T_ERR_STATE, "m2t_forward: keep_activations != 0 on an inference plan (option \"inference\"): it keeps nothing");
  hipStream_t st = (hipStream_t)stream;
  F32FastGuard f32_fast_guard(p->use_fp32_fast);
  const m2t_sched& sc = p->sc;
  const m2t_plan_handles& hd = p->hd;
  char* const ws = (char*)workspace;
  auto pk = [&](long long off) { return ws + hd.packed + (size_t)off * p->esz; };      // a packed weight
  const int dt = p->dt, B = p->B, H = p->H, W = p->W, s = p->scale;
  const long long BP = (long long)B * p->P;
  // a training plan keeps every activation whatever keep_activations says; on an inference plan the regions the forward never reads
  // are absent: region_ptr() hands the kernels a null pointer for them (on a training plan every region is present)
  // (re-packing on the side stream under the head conv was measured: -0.4 %, both kernels are bound by workgroup launch rate)
  {
    // the plain / transposed copies of the C >= 64 qkv weights are read only by the unfused projection GEMMs (forward / data gradient):
    // with the fused attention kernels in force (the bf16 default) they are not packed.  A change of either option invalidates the
    // activations (m2t_set_option), so the backward pass always meets the packs of the options it runs under
    const char* blocks = ws + hd.pack_blocks;
    const m2t_pack_desc* pdescs = (const m2t_pack_desc*)(ws + hd.pack_descs);
    const int n0 = p->pack_nb_base + (sc.need_copy ? p->pack_nb_copy : 0) + ((sc.need_copy && sc.need_tr) ? p->pack_nb_tr : 0);
    CK(launch_pack(dt, params, ws + hd.packed, pdescs, blocks, n0, st));
    if (sc.need_tr && !sc.need_copy)
      CK(launch_pack(dt, params, ws + hd.packed, pdescs, blocks + (size_t)(p->pack_nb_base + p->pack_nb_copy) * 2 * sizeof(int), p->pack_nb_tr, st));
  }
  CK(launch_head_conv_fwd(dt, x, params + hd.head_w, params + hd.head_b, ws + hd.X[0], B, p->H0, p->W0, H, W, st));
  int stat_partials = 0;
  for (int b = 0; b < p->nb; ++b) {
    const m2t_block_handles& bh = hd.blk[b];
    void* const Xres = ws + hd.X[b];                          // the block input: the residual of the block's conv
    void* X = Xres;                                           // ... and what the branches normalise
    float* mean = (float*)(ws + bh.mean);
    float* rstd = (float*)(ws + bh.rstd);
    void* xc = ws + bh.xc;
    if (p->local_norm > 0) {
      // local statistics + apply -> xn; the launches below are today's, on xn with the identity record: (xn - 0) * 1 is xn on every bit
      CK(launch_local_norm(dt, Xres, ws + hd.lnsum, ws + hd.xn, B, H, W, p->local_norm, st));
      X = ws + hd.xn;
      mean = (float*)(ws + hd.norm_id);
      rstd = mean + (size_t)B * 64;
    } else if (stat_partials > 0) {
      // statistics of the block input: left as per-segment partials by the previous block's conv (bf16, row-streaming), else two stages
      CK(launch_instnorm_finalize((const float*)(ws + hd.norm_part), mean, rstd, B, stat_partials, st));
    } else {
      CK(launch_instnorm_stats(dt, X, mean, rstd, (float*)(ws + hd.norm_part), B, (int)p->P, st));
    }
    for (int i = 0; i < 4; ++i) {
      const int C = BR_C[i], L = BR_L[i];
      const int h = H >> L, w = W >> L;
      const long long M = (long long)B * h * w;
      void* d = region_ptr(ws, bh.d[i]);
      void* qkv = region_ptr(ws, bh.qkv[i]);
      const float* rh = params + bh.rel_h[i];
      const float* rw = params + bh.rel_w[i];
      void* xc_i = (char*)xc + (size_t)i * BP * 16 * p->esz;       // chunk i of the P64 concat buffer: a dense plane
      if (sc.c16_fused_fwd && i == 0) {
        // x1 = attn1(norm(x)[chunk 0]) + norm(x)[chunk 0] (:135-139): one launch, d1 and qkv1 written for the backward
        CK(launch_window_attn_fused_c16_fwd(X, mean, rstd, pk(bh.w[0]), rh, rw, d, sc.stores_qkv1 ? qkv : nullptr, xc_i, 16, 0, B, h, w, st));
        continue;
      }
      // C = 64: qkv is written for the backward pass unless that recomputes it
      void* qkv_out = (C == 64 && !sc.stores_qkv2) ? nullptr : qkv;      // (inference plan: qkv itself is null on the fused paths)
      if (sc.prep_in_fwd && C >= 64) {
        // branch_prep (norm apply + mix + DWT^L), the qkv projection, the window attention and IWT^L / residual in one kernel
        const void* xn_i = (const char*)X + (size_t)i * BP * 16 * p->esz;
        const void* xprev = (const char*)xc + (size_t)(i - 1) * BP * 16 * p->esz;
        if (C == 256 && sc.fwd2 != 0)      // more windows than CUs: the kernels that put two windows on a CU (k_attn_fwd2.hip)
          CK(launch_window_attn_fused_prep_fwd2(xn_i, xprev, mean, rstd, i, ws + hd.xin, d, pk(bh.wF[i]), rh, rw, qkv, xc_i, region_ptr(ws, hd.vring), B, h, w, sc.fwd2, st));
        else
          CK(launch_window_attn_fused_prep_fwd(xn_i, xprev, mean, rstd, i, ws + hd.xin, d, pk(bh.wF[i]), rh, rw, qkv_out, xc_i, B, h, w, C, L, st));
        continue;
      }
      CK(launch_branch_prep(dt, L, X, mean, rstd, xc, i, ws + hd.xin, d, B, H, W, st));
      if (sc.c64_fused_fwd && C >= 64) {
        // qkv projection + window attention + IWT^L / residual in one kernel
        CK(launch_window_attn_fused_fwd(d, pk(bh.wF[i]), rh, rw, qkv_out, xc_i, 16, 0, ws + hd.xin, 16, B, h, w, C, L, st));
        continue;
      }
      m2t_gemm_args ga{};
      ga.A = d; ga.lda = C; ga.W = pk(bh.w[i]);
      ga.Y = qkv; ga.ldy = 3 * C; ga.M = M; ga.N = 3 * C; ga.K = C;
      { M2TProfScope ps(M2T_PROF_GEMM_QKV, st); CK(launch_gemm_nt(dt, M2T_A_PLAIN, M2T_E_PLAIN, ga, st)); }
      if (i == 0) {
        // x1 = attn1(x1) + x1 written straight into the concat buffer (:139,163)
        CK(launch_window_attn_fwd(dt, qkv, rh, rw, xc_i, 16, 0, d, 16, B, h, w, C, st));
      } else {
        // x_k = IWT^L(attn_k(.)) + x_k_in written straight into the concat buffer (:145,153,161,163)
        CK(launch_window_attn_fwd(dt, qkv, rh, rw, xc_i, 16, 0, ws + hd.xin, 16, B, h, w, C, st, L));
      }
    }
    // x = feed_forward(xc) + x (:164); the last block also folds in `res + x` (:70)
    { M2TProfScope ps(M2T_PROF_CONV3_FWD, st);
      // (local_norm: the next block takes no global statistics, so the conv leaves no partials)
      stat_partials = (b < p->nb - 1 && p->local_norm == 0) ? conv3x3_c64_stat_partials(dt, B, H, W, sc.conv_variant) : 0;
      CK(launch_conv3x3_c64(dt, xc, pk(bh.wf), params + bh.ffb, Xres, (b == p->nb - 1) ? ws + hd.X[0] : nullptr, ws + hd.X[b + 1], B, H, W, st,
                            pk(bh.wfR), ws + hd.zero_page, sc.conv_variant, stat_partials > 0 ? (float*)(ws + hd.norm_part) : nullptr)); }
  }
  void* Y = ws + hd.X[p->nb];
  const int r0 = (s == 4) ? 2 : s;
  const float* wlast = params + hd.wlast;
  float* srpre = (float*)(ws + hd.srpre);
  if (sc.tail_fwd == TAIL_FWD_X23_STREAM) {
    M2TProfScope ps(M2T_PROF_TAIL_FWD_FUSED, st);
    CK(launch_tail_fwd_stream(Y, 1, pk(hd.t0), params + hd.tail0_b, wlast, srpre, B, H, W, r0, 0, st));
  } else {
    { M2TProfScope ps(M2T_PROF_TAIL_GEMM, st);
      CK(launch_tail_expand(dt, Y, pk(hd.t0), params + hd.tail0_b, ws + hd.t1act, region_ptr(ws, hd.t1der), BP, H, W, r0, true, st)); }
    if (sc.tail_fwd == TAIL_FWD_STREAM) {
      M2TProfScope ps(M2T_PROF_TAIL_FWD_FUSED, st);
      CK(launch_tail_fwd_stream(ws + hd.t1act, 0, pk(hd.t3), params + hd.tail3_b, wlast, srpre, B, 2 * H, 2 * W, 2, 0, st));
    } else if (sc.tail_fwd == TAIL_FWD_TILE) {
      M2TProfScope ps(M2T_PROF_TAIL_FWD_FUSED, st);
      CK(launch_tail_fwd_fused(ws + hd.t1act, pk(hd.t3), params + hd.tail3_b, wlast, srpre, B, p->Hsp, p->Wsp, st));
    } else {
      if (s == 4) {
        M2TProfScope ps(M2T_PROF_TAIL_GEMM, st);
        CK(launch_tail_expand(dt, ws + hd.t1act, pk(hd.t3), params + hd.tail3_b, ws + hd.t2act, region_ptr(ws, hd.t2der), BP * 4, 2 * H, 2 * W, 2, false, st));
      }
      M2TProfScope ps(M2T_PROF_FINAL_FWD, st);
      CK(launch_final_conv_fwd(dt, ws + (s == 4 ? hd.t2act : hd.t1act), wlast, srpre, B, p->Hsp, p->Wsp, st));
    }
  }
  if (sr) CK(launch_clamp_l1(srpre, nullptr, sr, nullptr, nullptr, nullptr, B, p->Hsp, p->Wsp, p->Hs, p->Ws, rgb_range, 0.f, 0.f, st));
  if (p->health > 0 && p->health_on) CK(health_record(p, 0, sr, ws, st));      // the forward rows, behind the last kernel
  p->have_acts = !p->inference;      // an inference forward leaves neither activations nor a seed
  p->have_seed = false;
  p->l1_deferred = false;
  return 0;
}

// The pixel-loss family (m2t_pixel_loss.h: l1, mse, charbonnier, smooth_l1 -- reference losses.py:225-230, :287-297).  The kind only
// selects the per-pixel function inside the kernel that takes the loss; state rules, launches and the schedule are those of the L1 loss.
static int pixel_loss_request(const char* who, int kind, float param, float weight, double divisor, M2TPixelLoss* pl) {
  if (!m2t_pixel_loss_make(kind, param, (float)((double)weight / divisor), pl)) {
    char msg[200];
    if (kind < 0 || kind >= M2T_PL_KINDS) snprintf(msg, sizeof msg, "%s: unknown pixel-loss kind %d (0 l1, 1 mse, 2 charbonnier, 3 smooth_l1)", who, kind);
    else if (kind == M2T_PL_CHARBONNIER) snprintf(msg, sizeof msg, "%s: charbonnier needs a finite eps > 0, got %g", who, (double)param);
    else snprintf(msg, sizeof msg, "%s: smooth_l1 needs a finite beta > 0, got %g (beta = 0 is the l1 loss: use kind l1)", who, (double)param);
    return m2t_set_error(M2T_ERR_ARG, msg);
  }
  return 0;
}

extern "C" int m2t_pixel_loss(m2t_plan* p, int kind, float param, const float* hr, float weight, double divisor, float rgb_range,
                              float* loss_out, void* workspace, void* stream) {
  if (!p || !hr || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_pixel_loss: null argument");
  M2TPixelLoss pl;
  CK(pixel_loss_request("m2t_pixel_loss", kind, param, weight, divisor, &pl));
  CK(refuse_inference(p, "m2t_pixel_loss"));
  if (!p->have_acts) return m2t_set_error(M2T_ERR_STATE, "m2t_pixel_loss: call m2t_forward first");
  char* const ws = (char*)workspace;
  CK(launch_clamp_l1((const float*)(ws + p->hd.srpre), hr, nullptr, (float*)(ws + p->hd.gpre), (float*)(ws + p->hd.loss_part), loss_out,
                     p->B, p->Hsp, p->Wsp, p->Hs, p->Ws, rgb_range, pl.loss_scale, pl.gscale, (hipStream_t)stream, pl.kind, pl.param, pl.f0, pl.f1));
  p->have_seed = true;
  p->l1_deferred = false;
  return 0;
}
extern "C" int m2t_l1_loss(m2t_plan* p, const float* hr, float lambda_l1, double divisor, float rgb_range,
                           float* loss_out, void* workspace, void* stream) {
  return m2t_pixel_loss(p, M2T_PL_L1, 0.f, hr, lambda_l1, divisor, rgb_range, loss_out, workspace, stream);
}

// The same loss and seed, produced INSIDE the next m2t_backward: on the bf16 x4 path the clamp + loss seed are taken by the fused tail
// backward while it stages its g(sr) halo (the pre-clamp output is read there instead of a stored seed: one 150 MB pass and two
// launches fewer per step); everywhere else m2t_backward simply runs m2t_pixel_loss's kernel first.  hr must stay valid until then.
extern "C" int m2t_pixel_loss_deferred(m2t_plan* p, int kind, float param, const float* hr, float weight, double divisor, float rgb_range,
                                       float* loss_out, void* workspace, void* stream) {
  (void)stream;
  if (!p || !hr || !workspace || !loss_out) return m2t_set_error(M2T_ERR_ARG, "m2t_pixel_loss_deferred: null argument");
  M2TPixelLoss pl;
  CK(pixel_loss_request("m2t_pixel_loss_deferred", kind, param, weight, divisor, &pl));
  CK(refuse_inference(p, "m2t_pixel_loss_deferred"));
  if (!p->have_acts) return m2t_set_error(M2T_ERR_STATE, "m2t_pixel_loss_deferred: call m2t_forward first");
  p->l1_hr = hr; p->l1_loss_out = loss_out; p->l1_sc = pl.loss_scale; p->l1_R = rgb_range; p->l1_pl = pl;
  p->l1_deferred = true;
  p->have_seed = true;
  return 0;
}
extern "C" int m2t_l1_loss_deferred(m2t_plan* p, const float* hr, float lambda_l1, double divisor, float rgb_range,
                                    float* loss_out, void* workspace, void* stream) {
  return m2t_pixel_loss_deferred(p, M2T_PL_L1, 0.f, hr, lambda_l1, divisor, rgb_range, loss_out, workspace, stream);
}

// upstream gradient -> gradient of the padded pre-clamp output (clamp mask, zero outside the crop)
__global__ void __launch_bounds__(256) seed_from_grad_kernel(const float* __restrict__ pre, const float* __restrict__ gsr,
                                                             float* __restrict__ gpre, int B, int Hp, int Wp, int Hs, int Ws, float R) {
  const long long total = (long long)B * 3 * Hp * Wp;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(t % Wp);
    long long q = t / Wp;
    const int y = (int)(q % Hp);
    const long long bc = q / Hp;
    float g = 0.f;
    if (y < Hs && x < Ws) {
      const float v = pre[t];
      if (v >= 0.f && v <= R) g = gsr[(bc * Hs + y) * Ws + x];
    }
    gpre[t] = g;
  }
}
extern "C" int m2t_set_output_grad(m2t_plan* p, const float* g_sr, float rgb_range, void* workspace, void* stream) {
  if (!p || !g_sr || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_set_output_grad: null argument");
  CK(refuse_inference(p, "m2t_set_output_grad"));
  if (!p->have_acts) return m2t_set_error(M2T_ERR_STATE, "m2t_set_output_grad: call m2t_forward first");
  char* const ws = (char*)workspace;
  const long long total = (long long)p->B * 3 * p->Hsp * p->Wsp;
  hipLaunchKernelGGL(seed_from_grad_kernel, dim3((unsigned)std::min<long long>(ceil_divll(total, 256), 4096)), dim3(256), 0,
                     (hipStream_t)stream, (const float*)(ws + p->hd.srpre), g_sr, (float*)(ws + p->hd.gpre), p->B, p->Hsp, p->Wsp,
                     p->Hs, p->Ws, rgb_range);
  M2T_LAUNCH_CHECK();
  p->have_seed = true;
  p->l1_deferred = false;
  return 0;
}

// adds scale * g into the materialised seed: sample b's [3][gh][gw] block lands at its crop origin (crops_host int[B][2] = (row0, col0), or
// NULL: (0, 0)), through the same clamp mask and padded layout as m2t_set_output_grad (the opt-in differentiable SemanticLoss)
extern "C" int m2t_add_output_grad(m2t_plan* p, const float* g, int gh, int gw, const int* crops_host, float scale, float rgb_range,
                                   void* workspace, void* stream) {
  if (!p || !g || !workspace || gh < 1 || gw < 1) return m2t_set_error(M2T_ERR_ARG, "m2t_add_output_grad: null / bad argument");
  CK(refuse_inference(p, "m2t_add_output_grad"));
  if (!p->have_acts || !p->have_seed || p->l1_deferred)
    return m2t_set_error(M2T_ERR_STATE, "m2t_add_output_grad: needs a materialised seed (m2t_l1_loss / m2t_pixel_loss or m2t_set_output_grad)");
  for (int b = 0; b < p->B; ++b) {
    const int y0 = crops_host ? crops_host[2 * b] : 0, x0 = crops_host ? crops_host[2 * b + 1] : 0;
    if (y0 < 0 || x0 < 0 || y0 + gh > p->Hs || x0 + gw > p->Ws) return m2t_set_error(M2T_ERR_ARG, "m2t_add_output_grad: block outside the image");
  }
  char* const ws = (char*)workspace;
  const long long img = 3LL * p->Hsp * p->Wsp, blk = 3LL * gh * gw;
  for (int b0 = 0; b0 < p->B; b0 += 64) {
    const int nb = std::min(64, p->B - b0);
    M2TCropOrigins org{};
    for (int b = 0; b < nb; ++b) {
      org.y0[b] = crops_host ? crops_host[2 * (b0 + b)] : 0;
      org.x0[b] = crops_host ? crops_host[2 * (b0 + b) + 1] : 0;
    }
    CK(launch_add_output_grad((const float*)(ws + p->hd.srpre) + b0 * img, g + b0 * blk, (float*)(ws + p->hd.gpre) + b0 * img, nb, p->Hsp, p->Wsp,
                              gh, gw, org, scale, rgb_range, (hipStream_t)stream));
  }
  return 0;
}

// ---- the optional loss terms on the forward's pre-clamp output, each added into the materialised seed -------------------------------
// m2t_<term>_loss runs the routine of m2t_<term>_loss_tensor on ws:srpre (padded Hsp x Wsp, image in the top-left Hs x Ws) and ws:gpre.
// Scratch is the caller's: no plan option, no workspace region.  Every entry makes its refusals in one order: 1 null, 2 finite numbers,
// 3 the term's own argument rule, 4 size, 5 batch cap, 6 the term's own state rule, 7 the seed state (that of m2t_add_output_grad).
// loss_entry_args is 1 + 2 (m2t_vgg_loss leaves its numbers to vgg_check_common), loss_entry_seed is 5 .. 7 and hands back where the term
// reads and adds; 3, 4 and the decision of 6 stay in the entry.  `who` is the entry's __func__.
struct LossSeed { const float* x; long long xs_img; int xs_row; float* gx; };

static int loss_entry_args(const char* who, bool any_null, float rgb_range, double divisor, float weight, double more = 1.0,
                           const char* rule = "rgb_range and divisor must be finite numbers > 0, weight finite") {
  if (any_null) return m2t_set_error_at(M2T_ERR_ARG, who, "null argument");
  if (!(rgb_range > 0.f) || !std::isfinite(rgb_range) || !(divisor > 0.0) || !std::isfinite(divisor) || !std::isfinite(weight) ||
      !(more > 0.0) || !std::isfinite(more))
    return m2t_set_error_at(M2T_ERR_ARG, who, rule);
  return 0;
}

static int loss_entry_seed(const char* who, const m2t_plan* p, bool batch_ok, const char* batch_cap, void* workspace, LossSeed* s,
                           const char* term_state_refusal = nullptr) {
  if (!batch_ok) return m2t_set_error_at(M2T_ERR_ARG, who, batch_cap);
  CK(refuse_inference(p, who));
  if (term_state_refusal) return m2t_set_error_at(M2T_ERR_STATE, who, term_state_refusal);
  if (!p->have_acts || !p->have_seed || p->l1_deferred)
    return m2t_set_error_at(M2T_ERR_STATE, who, "needs a materialised seed (m2t_l1_loss / m2t_pixel_loss or m2t_set_output_grad)");
  char* const ws = (char*)workspace;
  *s = LossSeed{(const float*)(ws + p->hd.srpre), 3LL * p->Hsp * p->Wsp, p->Wsp, (float*)(ws + p->hd.gpre)};
  return 0;
}

// weight * (1 - mean SSIM) (k_ssim_loss.hip; losses.py:8, utils.py:232-234)
extern "C" int m2t_ssim_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, float* loss_out, int accumulate,
                             void* scratch, void* workspace, void* stream) {
  CK(loss_entry_args(__func__, !p || !hr || !loss_out || !scratch || !workspace, rgb_range, divisor, weight));
  if (p->Hs < 11 || p->Ws < 11) return m2t_set_error_at(M2T_ERR_ARG, __func__, "the SR image is smaller than the 11 x 11 window");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B * 3 <= 65535, "batch too large (B * 3 <= 65535)", workspace, &s));
  return launch_ssim_loss(s.x, hr, p->B, 3, p->Hs, p->Ws, s.xs_img, s.xs_row, rgb_range, 1, (double)weight / divisor, s.gx, loss_out,
                          accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}

// weight * (1 - mean MS-SSIM) (k_msssim_loss.hip; include/m2t_msssim.h)
extern "C" int m2t_msssim_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, float* loss_out,
                               int accumulate, void* scratch, void* workspace, void* stream) {
  CK(loss_entry_args(__func__, !p || !hr || !loss_out || !scratch || !workspace, rgb_range, divisor, weight));
  if (!msssim_loss_size_supported(p->Hs, p->Ws))
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "the SR height and width must be larger than 160 (five levels under the 11-tap window)");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B * 3 <= 65535, "batch too large (B * 3 <= 65535)", workspace, &s));
  return launch_msssim_loss(s.x, hr, p->B, 3, p->Hs, p->Ws, s.xs_img, s.xs_row, rgb_range, 1, (double)weight / divisor, s.gx, loss_out,
                            nullptr, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}

// weight * (1 - mean VIF) (k_vif_loss.hip; include/m2t_vif.h)
extern "C" int m2t_vif_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, double sigma_n_sq,
                            float* loss_out, int accumulate, void* scratch, void* workspace, void* stream) {
  CK(loss_entry_args(__func__, !p || !hr || !loss_out || !scratch || !workspace, rgb_range, divisor, weight, sigma_n_sq,
                     "rgb_range, divisor and sigma_n_sq must be finite numbers > 0, weight finite"));
  if (!vif_loss_size_supported(p->Hs, p->Ws))
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "the SR height and width must be at least 41 (four scales under the 17 / 9 / 5 / 3-tap windows)");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B <= 65535, "batch too large (B <= 65535)", workspace, &s));
  return launch_vif_loss(s.x, hr, p->B, 3, p->Hs, p->Ws, s.xs_img, s.xs_row, rgb_range, sigma_n_sq, 1, (double)weight / divisor, s.gx,
                         loss_out, nullptr, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}

// weight * mean GMSD (k_gmsd_loss.hip; include/m2t_gmsd.h)
extern "C" int m2t_gmsd_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, float* loss_out, int accumulate,
                             void* scratch, void* workspace, void* stream) {
  CK(loss_entry_args(__func__, !p || !hr || !loss_out || !scratch || !workspace, rgb_range, divisor, weight));
  if (!gmsd_loss_size_supported(p->Hs, p->Ws))
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "the SR height and width must be at least 2 (one 2 x 2 cell)");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B <= 65535, "batch too large (B <= 65535)", workspace, &s));
  return launch_gmsd_loss(s.x, hr, p->B, 3, p->Hs, p->Ws, s.xs_img, s.xs_row, rgb_range, 1, (double)weight / divisor, s.gx, loss_out,
                          nullptr, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}

// weight * mean over the coefficients of sum_band w_band rho(c_band) on an undecimated wavelet transform (k_wavelet_loss.hip;
// include/m2t_wavelet.h)
extern "C" int m2t_wavelet_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, const double* lo,
                                const double* hi, int taps, int levels, const double* band_weights, double eps, float* loss_out,
                                int accumulate, void* scratch, void* workspace, void* stream) {
  CK(loss_entry_args(__func__, !p || !hr || !lo || !hi || !loss_out || !scratch || !workspace, rgb_range, divisor, weight));
  if (const char* r = wavelet_filter_refusal(lo, hi, taps, levels, band_weights, eps)) return m2t_set_error_at(M2T_ERR_ARG, __func__, r);
  if (p->Hs < ((taps - 1) << (levels - 1)) + 1 || p->Ws < ((taps - 1) << (levels - 1)) + 1)
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "the SR height and width must be at least (taps - 1) * 2^(levels - 1) + 1");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B * 3 <= 65535, "batch too large (B * 3 <= 65535)", workspace, &s));
  return launch_wavelet_loss(s.x, hr, p->B, 3, p->Hs, p->Ws, s.xs_img, s.xs_row, rgb_range, 1, (double)weight / divisor, lo, hi, taps,
                             levels, band_weights, eps, nullptr, s.gx, loss_out, nullptr, accumulate ? 1 : 0, scratch,
                             (hipStream_t)stream);
}

// weight * mean rho((D clamp(sr) - lr) / R), D the bicubic down-sampler of the plan's scale (k_consistency.hip; include/m2t_consistency.h).
// The target is the step's own LR batch, not hr.
extern "C" int m2t_consistency_loss(m2t_plan* p, const float* lr, float weight, double divisor, float rgb_range, double eps, float* loss_out,
                                    int accumulate, void* scratch, void* workspace, void* stream) {
  CK(loss_entry_args(__func__, !p || !lr || !loss_out || !scratch || !workspace, rgb_range, divisor, weight));
  if (!(eps >= 0.0) || !std::isfinite(eps)) return m2t_set_error_at(M2T_ERR_ARG, __func__, "eps must be a finite number >= 0");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B * 3 <= 65535, "batch too large (B * 3 <= 65535)", workspace, &s));
  return launch_consistency_loss(s.x, lr, p->B, 3, p->H0, p->W0, p->scale, s.xs_img, s.xs_row, rgb_range, 1, eps, (double)weight / divisor,
                                 s.gx, loss_out, nullptr, accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}

// weight * sum_k w_k mean(rho(F_k(sr) - F_k(hr))) on VGG19 features (k_vgg.hip, m2t_vgg.hip; include/m2t_perceptual.h).  The tower's
// workspace is the caller's.
extern "C" int m2t_vgg_loss(m2t_plan* p, const m2t_vgg* v, const float* hr, float weight, double divisor, float rgb_range, int kind,
                            float param, const double* tap_weights, float* loss_out, int accumulate, void* vgg_workspace, void* workspace,
                            void* stream) {
  if (!p || !v || !hr || !loss_out || !vgg_workspace || !workspace) return m2t_set_error_at(M2T_ERR_ARG, __func__, "null argument");
  if (!(divisor > 0.0) || !std::isfinite(divisor)) return m2t_set_error_at(M2T_ERR_ARG, __func__, "divisor must be a finite number > 0");
  CK(vgg_check_common(__func__, tap_weights, (double)weight, rgb_range, kind, param));
  if (!vgg_size_supported(p->Hs, p->Ws))
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "the SR height and width must be at least 16 (four 2 x 2 pools before relu5_1)");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B <= 32767, "batch too large (B <= 32767)", workspace, &s,
                     vgg_loaded(v) ? nullptr : "call m2t_vgg_load_weights first (no VGG19 weights ship with the library)"));
  return launch_vgg_loss(v, s.x, hr, p->B, 3, p->Hs, p->Ws, s.xs_img, s.xs_row, rgb_range, 1, kind, param, tap_weights, (double)weight,
                         divisor, s.gx, loss_out, nullptr, accumulate ? 1 : 0, vgg_workspace, (hipStream_t)stream);
}

// weight * mean |rfft2(d)| (k_fft_loss.hip; include/m2t_spectral.h)
extern "C" int m2t_fft_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, int norm, float* loss_out,
                            int accumulate, void* scratch, void* workspace, void* stream) {
  CK(loss_entry_args(__func__, !p || !hr || !loss_out || !scratch || !workspace, rgb_range, divisor, weight));
  if (norm != 0 && norm != 1) return m2t_set_error_at(M2T_ERR_ARG, __func__, "norm must be 0 (backward) or 1 (ortho)");
  if (!fft_loss_size_supported(p->Hs, p->Ws))
    return m2t_set_error_at(M2T_ERR_ARG, __func__, "the SR height and width must be even, 8 .. 2048 and of the form 2^a * 3^b");
  LossSeed s;
  CK(loss_entry_seed(__func__, p, p->B * 3 <= 65535, "batch too large (B * 3 <= 65535)", workspace, &s));
  return launch_fft_loss(s.x, hr, p->B, 3, p->Hs, p->Ws, s.xs_img, s.xs_row, rgb_range, 1, norm, (double)weight / divisor, s.gx, loss_out,
                         accumulate ? 1 : 0, scratch, (hipStream_t)stream);
}

// Two-stream backward.  The data-gradient chain (what the next kernel needs) runs on the
// caller's stream; everything that only produces PARAMETER gradients (weight/bias gradients,
// slab reductions, rel-pos reductions) runs on the plan's side stream, forked/joined with
// events, because neither class of kernel fills 256 CUs on its own at these sizes.
// Hazards are closed explicitly: gqkv/relw are double-buffered and re-used only after the
// side stream's consumer of two branches ago has finished; a block's gy buffer is rewritten
// only after the side stream's conv-wgrad of the following block has read it.
//
// need_stage (m2t_backward_ex): n_blocks + 2 flags, head / body.b / tail, or NULL = every stage.  A clear flag drops that stage's
// parameter-gradient launches (the same ones debug_skip_side drops); the data-gradient chain runs down to the lowest stage needed,
// or to the input when gx != NULL.  Only the all-stages pass uses (and publishes) the plan's reduction table and its bucket events
// as it goes; any other pass reduces once at its end through its mask's own table and then records every bucket event.
static int backward_impl(m2t_plan* p, const float* params, const float* x, float* grads, float* gx_out,
                         const unsigned char* need_stage, void* workspace, void* stream) {
  const int nst = p->nb + 2;
  std::vector<unsigned char> need(nst, 1);
  if (need_stage)
    for (int i = 0; i < nst; ++i) need[i] = need_stage[i] ? 1 : 0;
  bool full = true, any = false, body_any = false;
  for (int i = 0; i < nst; ++i) { full = full && need[i]; any = any || need[i]; }
  for (int b = 0; b < p->nb; ++b) body_any = body_any || need[1 + b];
  const bool need_head = need[0] != 0, need_tail = need[nst - 1] != 0;
  // the data-gradient chain below the tail: needed by the head, a body stage or the input gradient
  const bool chain_body = gx_out || need_head || body_any;
  int lowest = p->nb;                        // lowest body block the chain reaches
  if (gx_out || need_head) lowest = 0;
  else for (int b = p->nb - 1; b >= 0; --b) if (need[1 + b]) lowest = b;
  F32FastGuard f32_fast_guard(p->use_fp32_fast);
  hipStream_t st = (hipStream_t)stream;
  if (p->ensure_side(st) != 0) return m2t_set_error(M2T_ERR_STATE, "m2t_backward: cannot create the side stream / events");
  hipStream_t sd = (p->use_side && any) ? p->side : st;      // no parameter gradient at all: no side-stream work
  const m2t_sched& sc = p->sc;
  const m2t_plan_handles& hd = p->hd;
  char* const ws = (char*)workspace;
  auto pk = [&](long long off) { return ws + hd.packed + (size_t)off * p->esz; };      // a packed weight
  size_t evi = 0;
  auto next_event = [&]() -> hipEvent_t { return p->events[(evi++) % p->events.size()]; };
  // option "fork_on_kernel": arm_fork() in front of the launch the fork follows; the event then rides on that dispatch as its stop
  // event (no marker packet between the kernel and its successor on the main stream).  fork() records as usual if nothing took it.
  hipEvent_t armed = nullptr;
  // the armed event is thread-local state that the NEXT timed launch of this thread takes: nothing armed by an earlier call (one that
  // returned early between arm_fork() and its launch) may leak into this pass, and nothing armed here may outlive it on any exit path
  g_m2t_fork_armed = nullptr;
  struct ForkArmGuard { ~ForkArmGuard() { g_m2t_fork_armed = nullptr; } } fork_arm_guard;
  hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap_status);
  const bool fork_on_kernel = sc.fork_on_kernel && cap_status == hipStreamCaptureStatusNone;   // an event-carrying dispatch is not a graph node
  auto arm_fork = [&]() {
    if (sd == st || !fork_on_kernel) return;
    armed = next_event();
    g_m2t_fork_armed = armed;
  };
  auto fork = [&]() {            // side stream continues from this point of the main stream
    if (sd == st) return;
    hipEvent_t e;
    if (armed && g_m2t_fork_armed == nullptr) e = armed;            // taken by the launch
    else { e = armed ? armed : next_event(); g_m2t_fork_armed = nullptr; (void)hipEventRecord(e, st); }
    armed = nullptr;
    (void)hipStreamWaitEvent(sd, e, 0);
  };
  auto side_marker = [&]() -> hipEvent_t {
    if (sd == st) return nullptr;
    hipEvent_t e = next_event();
    (void)hipEventRecord(e, sd);
    return e;
  };
  auto main_wait = [&](hipEvent_t e) { if (e) (void)hipStreamWaitEvent(st, e, 0); };
  // option "health" = 2: the backward rows, on the main stream behind the join of the side stream (both schedules end in it)
  auto health_backward = [&]() -> int {
    if (p->health < 2 || !p->health_on) return 0;
    return health_record(p, 1, full ? grads : nullptr, (char*)workspace, st);
  };

  const int dt = p->dt, B = p->B, H = p->H, W = p->W, s = p->scale;
  const long long BP = (long long)B * p->P;
  // ---- slab arena + deferred reductions (all on the side stream) ----
  float* arena = (float*)(ws + hd.arena);
  const m2t_red_desc* descs_dev = (const m2t_red_desc*)(ws + hd.red_descs);
  size_t arena_top = 0;
  std::vector<m2t_red_desc> descs;
  size_t flushed = 0;
  bool overflow = false;
  // returns nullptr (and the caller returns M2T_ERR_STATE through ARENA) BEFORE any kernel could write past the arena
  auto arena_alloc = [&](size_t nfloats) -> float* {
    arena_top = (arena_top + 63) & ~(size_t)63;
    if (arena_top + nfloats > p->arena_floats) { overflow = true; return nullptr; }
    float* ptr = arena + arena_top;
    arena_top += nfloats;
    return ptr;
  };
#define ARENA(var, nfloats)                                                                              \
  float* var = arena_alloc(nfloats);                                                                     \
  if (!var) return m2t_set_error(M2T_ERR_STATE, "m2t_backward: slab arena too small for this plan")
  auto defer = [&](const float* slab, long long dst_off, int ns, long long n, int perm, int p0, int p1, int p2) {
    m2t_red_desc d;
    d.src_off = (long long)(slab - arena); d.dst_off = dst_off; d.n = n; d.ns = ns; d.perm = perm; d.p0 = p0; d.p1 = p1; d.p2 = p2; d.pad_ = 0;
    descs.push_back(d);
  };
  auto table_fits = [&]() -> int {   // what was deferred so far fits the arena and the 512-entry device table
    if (overflow) return m2t_set_error(M2T_ERR_STATE, "m2t_backward: slab arena too small");
    if (descs.size() > 512) return m2t_set_error(M2T_ERR_STATE, "m2t_backward: too many deferred reductions");
    return 0;
  };
  size_t bucket_i = 0;
  auto mark_bucket_on = [&](hipStream_t rs) {   // the gradient range of bucket_i is final on stream rs from here on
    if (full && bucket_i < p->bucket_events.size() && p->red_uploaded) (void)hipEventRecord(p->bucket_events[bucket_i], rs);
    ++bucket_i;
  };
  auto mark_bucket = [&]() { mark_bucket_on(sd); };
  hipStream_t flush_stream = sd;
  auto flush = [&]() -> int {        // one launch reduces everything deferred since the last flush
    CK(table_fits());
    if (!full || !p->red_uploaded) return 0;  // first call (or a partial pass): table not on the device yet, reduced at the end
    const int cnt = (int)(descs.size() - flushed);
    int rc = launch_multi_reduce(arena, grads, descs_dev + flushed, cnt, flush_stream);
    flushed = descs.size();
    return rc;
  };
  float* relp = nullptr;
  const float* gpre = (const float*)(ws + hd.gpre);
  float* loss_part = (float*)(ws + hd.loss_part);
  int ns = 0;
  const int r0 = (s == 4) ? 2 : s;
  // ---- tail ----
  const float* wlast = params + hd.wlast;
  const bool skip = p->debug_skip_side || !need_tail;         // (the tail's parameter-gradient work)
  const bool skip_head = p->debug_skip_side || !need_head;
  hipStream_t tws = sd;      // tail weight gradients: side stream (same-box A/B: +0.5 % over the main stream)
  // a deferred L1 loss (m2t_l1_loss_deferred): inside the fused tail backward where that kernel runs in its recomputing form,
  // otherwise by m2t_l1_loss's own kernel, here -- on the main stream IN FRONT OF THE FIRST FORK: on the unfused tail path the tail
  // conv's weight gradient reads the seed on the side stream, which only orders itself behind what the fork event covers (round 5
  // enqueued it behind the fork: the side stream could read gpre while it was being written, or the previous step's seed)
  const bool l1_in_tail = p->l1_deferred && sc.l1_in_tail;
  if (p->l1_deferred && !l1_in_tail)
    CK(launch_clamp_l1((const float*)(ws + hd.srpre), p->l1_hr, nullptr, (float*)(ws + hd.gpre), loss_part, p->l1_loss_out,
                       p->B, p->Hsp, p->Wsp, p->Hs, p->Ws, p->l1_R, p->l1_sc, p->l1_pl.gscale, st, p->l1_pl.kind, p->l1_pl.param, p->l1_pl.f0,
                       p->l1_pl.f1));
  fork();
  hipEvent_t im2col_done = nullptr;           // head_cols is produced on the side stream; the head weight gradient may run on the main one
  if (!skip_head) { CK(launch_head_im2col(dt, x, ws + hd.head_cols, B, p->H0, p->W0, H, W, sd)); im2col_done = side_marker(); }
  void* Y = ws + hd.X[p->nb];
  if (sc.tail_bwd == TAIL_BWD_X23_STREAM) {
    // x2 / x3: the whole tail backward in one row-streaming launch (k_tail_bwd_stream.hip): g(body output) straight into gT
    const int N0 = 64 * r0 * r0;
    const int nb = tail_bwd_stream_blocks(B, H, W, r0);
    ARENA(swf, (size_t)nb * 32 * 64);
    ARENA(sw0, (size_t)nb * N0 * 64);
    ARENA(sb0, (size_t)nb * N0);
    { M2TProfScope ps(M2T_PROF_FINAL_DGRAD, st);
      CK(launch_tail_bwd_stream(gpre, wlast, Y, nullptr, pk(hd.t0T), params + hd.tail0_b, ws + hd.gT, swf, sw0, sb0, &ns, B, H, W, r0, 1, st)); }
    if (!skip) {
      defer(swf, hd.wlast, ns, 32 * 64, 3, 0, 0, 0);
      defer(sw0, hd.tail0_w, ns, (long long)N0 * 64, 2, 64, r0 * r0, 64);
      defer(sb0, hd.tail0_b, ns, N0, 2, 64, r0 * r0, 1);
    }
  } else if (sc.tail_bwd != TAIL_BWD_PLAIN) {
    // x4: one pass over the high-resolution tensors (k_tail_bwd.hip): tail conv dgrad + wgrad, GELU', tail.3 dgrad + wgrad
    const bool sbwd = sc.tail_bwd == TAIL_BWD_STREAM;      // (the streaming form always recomputes)
    const int nb = sbwd ? tail_bwd_stream_blocks(B, 2 * H, 2 * W, 2) : tail_bwd_fused_blocks(B, p->Hsp, p->Wsp);
    ARENA(swf, (size_t)nb * 32 * 64);
    ARENA(sw3, (size_t)nb * 256 * 64);
    ARENA(sb3, (size_t)nb * 256);
    { M2TProfScope ps(M2T_PROF_FINAL_DGRAD, st);
      const bool stored = sc.tail_bwd == TAIL_BWD_STORED;  // else the forward did not store gelu(t2) / gelu'(t2): recomputed per tile
      if (sbwd)
        CK(launch_tail_bwd_stream(gpre, wlast, ws + hd.t1act, ws + hd.t1der, pk(hd.t3T), params + hd.tail3_b, ws + hd.g_t1pre, swf, sw3, sb3, &ns,
                                  B, 2 * H, 2 * W, 2, 0, st));
      else
        CK(launch_tail_bwd_fused(gpre, wlast, stored ? ws + hd.t2act : nullptr, stored ? ws + hd.t2der : nullptr, ws + hd.t1act, ws + hd.t1der,
                                 pk(hd.t3T), params + hd.tail3_b, ws + hd.g_t1pre, swf, sw3, sb3, &ns, B, p->Hsp, p->Wsp, st,
                                 l1_in_tail ? (const float*)(ws + hd.srpre) : nullptr, p->l1_hr, loss_part, p->Hs, p->Ws, p->l1_R,
                                 p->l1_pl.gscale, sc.tail_bwd == TAIL_BWD_RC32 ? 32 : 16, p->l1_pl.kind, p->l1_pl.param, p->l1_pl.f0, p->l1_pl.f1)); }
    if (l1_in_tail) CK(launch_loss_finish(loss_part, ns, p->l1_sc, p->l1_loss_out, st));
    if (!skip) {
      defer(swf, hd.wlast, ns, 32 * 64, 3, 0, 0, 0);
      defer(sw3, hd.tail3_w, ns, 256 * 64, 2, 64, 4, 64);
      defer(sb3, hd.tail3_b, ns, 256, 2, 64, 4, 1);
    }
  } else {
    if (!skip) {
      ARENA(slabs, (size_t)1024 * 32 * 64);
      { M2TProfScope ps(M2T_PROF_FINAL_WGRAD, tws);
        CK(launch_final_conv_wgrad(dt, gpre, ws + (s == 4 ? hd.t2act : hd.t1act), slabs, &ns, B, p->Hsp, p->Wsp, tws)); }
      defer(slabs, hd.wlast, ns, 32 * 64, 3, 0, 0, 0);
    }
    { M2TProfScope ps(M2T_PROF_FINAL_DGRAD, st);
      CK(launch_final_conv_dgrad(dt, gpre, wlast, ws + (s == 4 ? hd.t2der : hd.t1der), ws + (s == 4 ? hd.g_t2pre : hd.g_t1pre), B, p->Hsp, p->Wsp, st)); }
    if (s == 4) {
      // tail.3: u = t1act W3^T + b3 (t1act = gelu(t1)), shuffled; g(t1) = (g_u W3) * t1der
      fork();
      ARENA(slabs, (size_t)wgrad_slab_count(BP * 4, 256, 64) * 256 * 64);
      ARENA(colp, (size_t)wgrad_slab_count(BP * 4, 256, 64) * 256);
      if (!skip) {
        m2t_wgrad_args wa{};
        wa.G = ws + hd.g_t2pre; wa.gmode = M2T_A_UNSHUF; wa.X = ws + hd.t1act; wa.ldx = 64; wa.xmode = M2T_A_PLAIN;
        wa.slabs = slabs; wa.bias_slabs = colp; wa.M = BP * 4; wa.N = 256; wa.K = 64; wa.H = 2 * H; wa.Wd = 2 * W; wa.r = 2; wa.C = 64;
        { M2TProfScope ps(M2T_PROF_TAIL_WGRAD, tws); CK(launch_wgrad_tn(dt, wa, &ns, tws)); }
        defer(slabs, hd.tail3_w, ns, 256 * 64, 2, 64, 4, 64);
        defer(colp, hd.tail3_b, ns, 256, 2, 64, 4, 1);   // bias gradient rode along in the wgrad kernel
      }
      m2t_gemm_args ga{};
      ga.A = ws + hd.g_t2pre; ga.W = pk(hd.t3T); ga.Y = ws + hd.g_t1pre; ga.ldy = 64;
      ga.aux = ws + hd.t1der; ga.ldaux = 64; ga.M = BP * 4; ga.N = 64; ga.K = 256;
      ga.H = 2 * H; ga.Wd = 2 * W; ga.r = 2; ga.C = 64;
      { M2TProfScope ps(M2T_PROF_TAIL_GEMM, st); CK(launch_gemm_nt(dt, M2T_A_UNSHUF, M2T_E_GELU_GRAD, ga, st)); }
    }
  }
  if (sc.tail_bwd != TAIL_BWD_X23_STREAM) {
    const int N0 = 64 * r0 * r0;
    fork();
    ARENA(slabs, (size_t)wgrad_slab_count(BP, N0, 64) * N0 * 64);
    ARENA(colp, (size_t)wgrad_slab_count(BP, N0, 64) * N0);
    if (!skip) {
      m2t_wgrad_args wa{};
      wa.G = ws + hd.g_t1pre; wa.gmode = M2T_A_UNSHUF; wa.X = Y; wa.ldx = M2T_LD_P64; wa.xmode = M2T_A_PLAIN;
      wa.slabs = slabs; wa.bias_slabs = colp; wa.M = BP; wa.N = N0; wa.K = 64; wa.H = H; wa.Wd = W; wa.r = r0; wa.C = 64;
      { M2TProfScope ps(M2T_PROF_TAIL_WGRAD, tws); CK(launch_wgrad_tn(dt, wa, &ns, tws)); }
      defer(slabs, hd.tail0_w, ns, (long long)N0 * 64, 2, 64, r0 * r0, 64);
      defer(colp, hd.tail0_b, ns, N0, 2, 64, r0 * r0, 1);
    }
    m2t_gemm_args ga{};
    ga.A = ws + hd.g_t1pre; ga.W = pk(hd.t0T); ga.Y = ws + hd.gT; ga.ldy = M2T_LD_P64;
    ga.M = BP; ga.N = 64; ga.K = N0; ga.H = H; ga.Wd = W; ga.r = r0; ga.C = 64;
    if (chain_body) { M2TProfScope ps(M2T_PROF_TAIL_GEMM, st); CK(launch_gemm_nt(dt, M2T_A_UNSHUF, M2T_E_PLAIN, ga, st)); }
  }
  if (sc.tail_bwd != TAIL_BWD_PLAIN) fork();     // the reduction (side stream) follows the main-stream producer
  CK(flush());
  mark_bucket();
  // ---- body, last block first.  gy = gradient of X[b+1] ----
  void* gy = ws + hd.gT;
  void* gnext[2] = {ws + hd.gA, ws + hd.gB};
  void* const gxc = ws + hd.gxc;
  void* const gn = ws + hd.gn;
  float* const norm_part = (float*)(ws + hd.norm_part);
  // Every event recorded on / waited for by the main stream costs a few microseconds of idle between two dependent kernels (the
  // backward's launches sit 4-7 us apart where such an operation lies between them, 0-1 us where none does): the block's side work
  // is therefore released with TWO forks (at the gate, and after the last branch), and its buffers are protected by ONE wait per
  // block -- for the side work of the block two back, which used the same buffer set.
  hipEvent_t block_done[2] = {nullptr, nullptr};
  hipEvent_t conv_done_prev = nullptr;      // side finished reading gy of the previously processed block
  // Side-stream schedule.  The two C = 256 attention kernels that open a block need a whole CU's LDS per workgroup
  // (k_attn_res.hip): any concurrent parameter-gradient kernel starves them until it has drained (measured:
  // 70 us instead of 25 us per launch); the C = 64 / C = 16 attention kernels run 2x slower next to a weight-
  // gradient GEMM.  So the block's side work is GATED behind the attention launch of branch `gate_branch`
  // (default 2 = behind both C = 256 launches): the conv / qkv weight gradients then run under the halo gathers, the
  // C = 64 / C = 16 attention (which lose less than the step gains), the data-gradient GEMMs and the norm backward.  Each branch has its own gqkv / win / relw
  // buffers, so the lag is harmless.
  const bool gated = p->gate_branch >= 0 && sd != st;
  const int gate = p->gate_branch;          // branch index after whose attention launch the block's side work is released
  for (int b = p->nb - 1; b >= lowest; --b) {
    const m2t_block_handles& bh = hd.blk[b];
    const bool skip = p->debug_skip_side || !need[1 + b];     // (this block's parameter-gradient work)
    void* X = ws + hd.X[b];
    float* mean = (float*)(ws + bh.mean);
    float* rstd = (float*)(ws + bh.rstd);
    void* xc = ws + bh.xc;
    bool norm_prered = false;                  // the InstanceNorm backward's first reduction stage rode in the C = 16 prep launch
    void* gy_blk = gy;
    const size_t* gqkv_off = hd.gqkv[b & 1]; const size_t* relw_off = hd.relw[b & 1]; const size_t* win_off = hd.win[b & 1];   // this block's buffer set
    main_wait(block_done[b & 1]);              // the side consumers of this buffer set (block b + 2) are done
    std::vector<int> pending;                  // branches whose side work waits for the block's second fork
    // feed_forward conv: weight / bias gradients on the side stream, data gradient on the main one
    auto side_conv = [&]() -> int {
      if (skip) return 0;
      ARENA(slabs, (size_t)256 * 9 * 64 * 64);
      ARENA(colp, (size_t)256 * 64);
      { M2TProfScope ps(M2T_PROF_CONV3_WGRAD, sd); CK(launch_conv3x3_c64_wgrad(dt, xc, gy_blk, slabs, colp, &ns, B, H, W, sd)); }
      defer(slabs, bh.ffw, ns, 9 * 64 * 64, 1, 64, 64, 0);
      defer(colp, bh.ffb, ns, 64, 0, 0, 0, 0);     // bias gradient rode along
      return 0;
    };
    auto fused_dgrad = [&](int i) -> bool {    // projection data gradient inside the attention backward kernel (k_attn_res.hip)
      return sc.fused_dgrad && BR_C[i] >= 64;
    };
    auto side_branch = [&](int i) -> int {     // qkv weight gradient + rel-pos partial reduction of branch i
      if (skip) return 0;
      const int C = BR_C[i], L = BR_L[i];
      const int h = H >> L, w = W >> L;
      const long long M = (long long)B * h * w;
      ARENA(slabs, (size_t)wgrad_slab_count(M, 3 * C, C) * 3 * C * C);
      // fused data gradient: the main chain never reads gqkv, so the overlap-add of dK|dV happens here, off the critical path
      if (fused_dgrad(i)) CK(launch_halo_gather(dt, ws + win_off[i], ws + gqkv_off[i], B, h, w, 2 * C, 3 * C, C, sd));
      m2t_wgrad_args wa{};
      wa.G = ws + gqkv_off[i]; wa.ldg = 3 * C; wa.gmode = M2T_A_PLAIN; wa.X = ws + bh.d[i]; wa.ldx = C; wa.xmode = M2T_A_PLAIN;
      wa.slabs = slabs; wa.M = M; wa.N = 3 * C; wa.K = C; wa.H = h; wa.Wd = w; wa.r = 1; wa.C = C; wa.halo_win = ws + win_off[i];
      wa.big_tiles = p->wgrad_big_tiles >= 0 ? p->wgrad_big_tiles : (M >= 24576 ? 256 : 0);
      { M2TProfScope ps(M2T_PROF_WGRAD_QKV, sd); CK(launch_wgrad_tn(dt, wa, &ns, sd)); }
      defer(slabs, bh.wqkv[i], ns, 3LL * C * C, 0, 0, 0, 0);
      ARENA(relp, (size_t)32 * 10 * C);
      int nsp = 0;
      CK(launch_rel_reduce1((float*)(ws + relw_off[i]), relp, (int)(M / 64), C, &nsp, sd));
      defer(relp, bh.rel_h[i], nsp, 10LL * C, 4, C, 0, 0);     // rel_h then rel_w are adjacent parameters
      return 0;
    };
    hipEvent_t conv_done = nullptr;
    // bf16: both gradients in one pass over gy on the main stream (the partials still reduce on the side stream: every block
    // forks at least once after this launch and before its flush)
    const bool fuse_conv = sc.fused_conv_bwd && !skip;
    if (fuse_conv) {
      ARENA(slabs, (size_t)256 * 9 * 64 * 64);
      ARENA(colp, (size_t)256 * 64);
      { M2TProfScope ps(M2T_PROF_CONV3_BWD, st);
        CK(launch_conv3x3_c64_bwd_fused(gy, xc, pk(bh.wfTR), gxc, slabs, colp, &ns, ws + hd.zero_page, B, H, W, st)); }
      defer(slabs, bh.ffw, ns, 9 * 64 * 64, 6, 64, 64, 0);    // slabs come as [tap][ic][oc]
      defer(colp, bh.ffb, ns, 64, 0, 0, 0, 0);
    } else if (!gated) {
      fork();
      CK(side_conv());
      conv_done = side_marker();
    }
    if (!fuse_conv)
    { M2TProfScope ps(M2T_PROF_CONV3_DGRAD, st);
      CK(launch_conv3x3_c64(dt, gy, pk(bh.wfT), nullptr, nullptr, nullptr, gxc, B, H, W, st, pk(bh.wfTR), ws + hd.zero_page, sc.conv_variant)); }
    for (int i = 3; i >= 0; --i) {
      const int C = BR_C[i], L = BR_L[i];
      const int h = H >> L, w = W >> L;
      const long long M = (long long)B * h * w;
      const void* qkv = ws + bh.qkv[i];
      const float* rh = params + bh.rel_h[i];
      const float* rw = params + bh.rel_w[i];
      void* gqkv = ws + gqkv_off[i];
      void* win = ws + win_off[i];
      float* relw = (float*)(ws + relw_off[i]);
      // gradient of IWT^L is DWT^L: applied while the kernel loads g_xc[chunk i]
      // dK|dV stay window-major in `win`; the fused tail kernel gathers them once per row, writes them back
      // into gqkv for the weight-gradient GEMM, multiplies by Wqkv and applies IWT / branch mixing.
      // (gathering inside the TILED GEMM / wgrad loaders, M2T_A_HALO, was measured slower: the gather is then
      //  repeated once per column-block.)
      const void* gxc_i = (const char*)gxc + (size_t)i * BP * 16 * p->esz;       // chunk i of the P64 gradient: a dense plane
      // bf16 C = 16 with "attn_bwd" = 3: the overlap-add, the projection data gradient and branch_prep_bwd are one kernel behind
      // the attention backward; it completes dK|dV in gqkv, so the branch's side work is released after it
      const bool c16_prep = C == 16 && sc.c16_prep;
      if (!gated && fused_dgrad(i)) arm_fork();
      // branch 4's branch_prep_bwd runs inside branch 3's attention backward (same level, same window grid): branch 4 then leaves its
      // own-window g_d rows in the second buffer set, and its prep launch is skipped below
      const bool pb_consumer = i == 2 && sc.prep_in_bwd;
      const bool pb_producer = i == 3 && sc.prep_in_bwd;
      if (fused_dgrad(i)) {
        M2TProfScope ps(C == 64 ? M2T_PROF_ATTN_BWD_64 : M2T_PROF_ATTN_BWD_256, st);
        const bool rc64 = C == 64 && sc.c64_recompute;
        CK(launch_window_attn_bwd_resident(qkv, rh, rw, gxc_i, 16, 0, gqkv, win, relw, B, h, w, C, L, st, pk(bh.wTF[i]),
                                           ws + (pb_producer ? hd.gd2 : hd.gd), ws + (pb_producer ? hd.gdwin2 : hd.gdwin),
                                           rc64 ? ws + bh.d[i] : nullptr, rc64 ? pk(bh.wF[i]) : nullptr,
                                           pb_consumer ? ws + hd.gd2 : nullptr, pb_consumer ? ws + hd.gdwin2 : nullptr,
                                           pb_consumer ? (const void*)((const char*)gxc + (size_t)(i + 1) * BP * 16 * p->esz) : nullptr,
                                           pb_consumer ? (void*)((char*)gn + (size_t)(i + 1) * BP * 16 * p->esz) : nullptr));
      } else if (C == 16 && sc.c16_recompute) {
        // qkv1 was not stored: recomputed inside the kernel from d1 (identical bits); then the halo overlap-add as usual
        { M2TProfScope ps(M2T_PROF_ATTN_BWD_16, st);
          CK(launch_window_attn_bwd_c16(nullptr, rh, rw, gxc_i, 16, 0, gqkv, win, relw, B, h, w, st, ws + bh.d[0], pk(bh.w[0]))); }
        if (!c16_prep) CK(launch_halo_gather(dt, win, gqkv, B, h, w, 2 * C, 3 * C, C, st));
      } else {
        CK(launch_window_attn_bwd(dt, qkv, rh, rw, gxc_i, 16, 0, gqkv, win, relw, B, h, w, C, st, L, !c16_prep, sc.resident_bwd));
      }
      auto release_side = [&]() -> int {
        if (!gated) {
          fork();
          CK(side_branch(i));
          if (i == 0) block_done[b & 1] = side_marker();
        } else if (i == gate) {
          fork();                              // the gate: the LDS-hungry attention kernels of this block are on their way
          // gated branches first, then the block's conv weight gradient (512 threads, 80 KB of LDS: +1.9 % over putting it
          // first, where it met the C = 64 attention)
          for (int j = 3; j >= gate; --j) CK(side_branch(j));
          if (!fuse_conv) {
            CK(side_conv());
            conv_done = side_marker();
          }
          if (i == 0) block_done[b & 1] = side_marker();
        } else if (i < gate) {
          pending.push_back(i);                // released together behind the last branch: one fork instead of one per branch
          if (i == 0) {
            fork();
            for (int j : pending) CK(side_branch(j));
            block_done[b & 1] = side_marker();
          }
        }
        return 0;
      };
      if (!c16_prep) CK(release_side());
      if (pb_producer) {
        // (nothing: the next attention backward applies this branch's branch_prep_bwd while it loads its output gradient)
      } else if (fused_dgrad(i)) {
        // own-window products are in gd; add the ring rows of the (<= 3) neighbouring windows to the border pixels
        CK(launch_branch_prep_bwd(dt, L, ws + hd.gd, gxc, gn, i, B, H, W, st, ws + hd.gdwin));
      } else if (c16_prep) {
        if (!gated) arm_fork();
        if (sc.norm_red_in_prep) {
          CK(launch_c16_dgrad_prep(gqkv, win, pk(bh.wT[0]), gxc, gn, B, H, W, st, X, mean, rstd, norm_part, (float*)(ws + hd.norm_part0)));
          norm_prered = true;
        } else {
          CK(launch_c16_dgrad_prep(gqkv, win, pk(bh.wT[0]), gxc, gn, B, H, W, st));
        }
        CK(release_side());
      } else {
        m2t_gemm_args ga{};
        ga.A = gqkv; ga.lda = 3 * C; ga.W = pk(bh.wT[i]);
        ga.Y = ws + hd.gd; ga.ldy = C; ga.M = M; ga.N = C; ga.K = 3 * C; ga.H = h; ga.Wd = w; ga.r = 1; ga.C = C; ga.halo_win = win;
        { M2TProfScope ps(M2T_PROF_GEMM_QKV_DGRAD, st); CK(launch_gemm_nt(dt, M2T_A_PLAIN, M2T_E_PLAIN, ga, st)); }
        CK(launch_branch_prep_bwd(dt, L, ws + hd.gd, gxc, gn, i, B, H, W, st));
      }
    }
    // block 0: the head's g(res) = g(X0) + g(Y) joins in the same pass and lands where the head weight gradient reads it
    void* gx = (b == 0) ? gxc : gnext[b & 1];
    // gx's buffer was the gy of block b+1: its conv-wgrad / colsum on the side stream must be done
    main_wait(conv_done_prev);
    CK(launch_instnorm_bwd(dt, gn, X, mean, rstd, gy, gx, norm_part, (float*)(ws + hd.norm_s), B, (int)p->P, st,
                           norm_prered ? (const float*)(ws + hd.norm_part0) : nullptr, H * (W / 16), (b == 0) ? ws + hd.gT : nullptr));
    conv_done_prev = conv_done;
    gy = gx;
    if ((b & 1) == 0) { CK(flush()); mark_bucket(); }
    else if (b == 1) CK(flush());      // (the step's last pair: its first half is reduced under block 0, so that what is left after the
                                       //  last data-gradient kernel is short -- the main stream idles until it is done)
  }
  // head: g(res) = g(X0) from the chain + g(Y) from `res + x`: added inside block 0's InstanceNorm backward (it wrote gxc)
  if (p->nb == 0 && chain_body) CK(launch_add(dt, gy, ws + hd.gT, gxc, BP * 64, st));
  // the input gradient: the head conv's adjoint over gxc = g(res), which nothing writes after this point
  if (gx_out) CK(launch_head_conv_dgrad(dt, gxc, params + hd.head_w, gx_out, B, p->H0, p->W0, H, W, st));
  // The end of the step is a serial chain: head weight gradient -> its reduction -> (the caller's) Adam.  In steady state it runs on the
  // MAIN stream behind the last data-gradient kernel: handing it to the side stream and back cost two cross-stream waits and a
  // queue position behind the last block pair's reduction (96 us between the last backward kernel and Adam, measured).
  const bool tail_on_main = full && p->red_uploaded && sd != st;
  hipStream_t hs = tail_on_main ? st : sd;
  if (!tail_on_main) fork();
  if (!skip_head) {
    // head conv: im2col'd input (made at the start of this backward, off the critical path) x output gradient
    const int nsl = wgrad_slab_count(BP, 64, 32);
    ARENA(slabs, (size_t)nsl * 64 * 32);
    ARENA(colp, (size_t)nsl * 64);
    m2t_wgrad_args wa{};
    wa.G = gxc; wa.ldg = M2T_LD_P64; wa.gmode = M2T_A_PLAIN; wa.X = ws + hd.head_cols; wa.ldx = 32; wa.xmode = M2T_A_PLAIN;
    wa.slabs = slabs; wa.bias_slabs = colp; wa.M = BP; wa.N = 64; wa.K = 32; wa.H = H; wa.Wd = W; wa.r = 1; wa.C = 64;
    if (hs == st) main_wait(im2col_done);      // (long since complete; the wait closes the hazard for every n_blocks)
    CK(launch_wgrad_tn(dt, wa, &ns, hs));
    defer(slabs, hd.head_w, ns, 64 * 32, 5, 32, 27, 0);
    defer(colp, hd.head_b, ns, 64, 0, 0, 0, 0);
  }
  CK(table_fits());
  if (!full) {
    // a partial pass: everything deferred is reduced here, through this mask's own table (uploaded once per mask and plan option set,
    // never the plan's published table, which stays the all-stages one); then every bucket event is recorded, so that
    // m2t_stream_wait_bucket after such a pass waits for the whole pass
    if (!descs.empty()) {
      m2t_plan::MaskTable& mt = p->mask_tables[need];
      if (!mt.uploaded) {
        if (cap_status != hipStreamCaptureStatusNone)
          return m2t_set_error(M2T_ERR_STATE, "m2t_backward_ex: the first pass of a stage mask cannot be captured (it uploads the mask's table)");
        if (!mt.dev) {
          hipError_t e = hipMalloc(&mt.dev, 512 * sizeof(m2t_red_desc));
          if (e != hipSuccess) { mt.dev = nullptr; return m2t_set_hip_error(e, __FILE__, __LINE__); }
        }
        mt.descs = descs;
        hipError_t e = hipMemcpyAsync(mt.dev, mt.descs.data(), descs.size() * sizeof(m2t_red_desc), hipMemcpyHostToDevice, sd);
        if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
        mt.uploaded = true;
      } else if (mt.descs.size() != descs.size()) {
        return m2t_set_error(M2T_ERR_STATE, "m2t_backward_ex: reduction table changed between steps");
      }
      CK(launch_multi_reduce(arena, grads, (const m2t_red_desc*)mt.dev, (int)descs.size(), sd));
    }
    for (auto e : p->bucket_events) (void)hipEventRecord(e, sd);
    main_wait(side_marker());
    CK(health_backward());         // (a partial pass: no grads row; a region it did not write keeps what it held)
    p->have_seed = false;
    p->l1_deferred = false;
    return 0;
  }
  const bool first_backward = !p->red_uploaded;
  if (!p->red_uploaded) {
    // first backward of this plan: publish the (step-invariant) descriptor table, then reduce everything
    p->red_descs = descs;
    hipError_t e = hipMemcpyAsync(ws + hd.red_descs, p->red_descs.data(), descs.size() * sizeof(m2t_red_desc), hipMemcpyHostToDevice, sd);
    if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
    p->red_uploaded = true;
    flushed = 0;
  } else if (p->red_descs.size() != descs.size()) {
    return m2t_set_error(M2T_ERR_STATE, "m2t_backward: reduction table changed between steps");
  }
  if (tail_on_main && !first_backward) {
    main_wait(side_marker());        // join first: everything the side stream still reduces; then the head's reduction on this stream
    flush_stream = st;
    CK(flush());
    mark_bucket_on(st);
  } else {
    CK(flush());
    mark_bucket();
  }
  if (first_backward)                // nothing was reduced before this point: every bucket completes here
    for (auto e : p->bucket_events) (void)hipEventRecord(e, sd);
  if (bucket_i != p->buckets.size()) return m2t_set_error(M2T_ERR_STATE, "m2t_backward: gradient bucket table out of step");
  if (!(tail_on_main && !first_backward)) main_wait(side_marker());          // join: every gradient is complete in main-stream order
  CK(health_backward());
  p->have_seed = false;
  p->l1_deferred = false;
  return 0;
}

extern "C" int m2t_backward(m2t_plan* p, const float* params, const float* x, float* grads, void* workspace,
                            void* stream) {
  if (!p || !params || !x || !grads || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_backward: null argument");
  CK(refuse_inference(p, "m2t_backward"));
  if (!p->have_acts || !p->have_seed)
    return m2t_set_error(M2T_ERR_STATE, "m2t_backward: needs m2t_forward and a seed (m2t_l1_loss / m2t_set_output_grad)");
  return backward_impl(p, params, x, grads, nullptr, nullptr, workspace, stream);
}

extern "C" int m2t_backward_ex(m2t_plan* p, const float* params, const float* x, float* grads, float* gx,
                               const unsigned char* need_stage, void* workspace, void* stream) {
  if (!p || !params || !workspace) return m2t_set_error(M2T_ERR_ARG, "m2t_backward_ex: null argument");
  bool any = false;
  for (int i = 0; i < p->nb + 2; ++i) any = any || !need_stage || need_stage[i];
  if (!any && !gx) return m2t_set_error(M2T_ERR_ARG, "m2t_backward_ex: nothing requested (no stage flag set and gx == NULL)");
  if (any && !grads) return m2t_set_error(M2T_ERR_ARG, "m2t_backward_ex: a stage flag is set but grads is NULL");
  if ((!need_stage || need_stage[0]) && !x) return m2t_set_error(M2T_ERR_ARG, "m2t_backward_ex: the head's gradient needs x");
  CK(refuse_inference(p, "m2t_backward_ex"));
  if (!p->have_acts || !p->have_seed)
    return m2t_set_error(M2T_ERR_STATE, "m2t_backward_ex: needs m2t_forward and a seed (m2t_l1_loss / m2t_set_output_grad)");
  return backward_impl(p, params, x, grads, gx, need_stage, workspace, stream);
}

extern "C" int m2t_stream_wait_bucket(m2t_plan* p, int bucket, void* stream) {
  if (!p || bucket < 0 || (size_t)bucket >= p->buckets.size()) return m2t_set_error(M2T_ERR_ARG, "m2t_stream_wait_bucket: bad bucket");
  CK(refuse_inference(p, "m2t_stream_wait_bucket"));
  if (p->bucket_events.size() != p->buckets.size()) return m2t_set_error(M2T_ERR_STATE, "m2t_stream_wait_bucket: call m2t_backward first");
  hipError_t e = hipStreamWaitEvent((hipStream_t)stream, p->bucket_events[bucket], 0);
  if (e != hipSuccess) return m2t_set_hip_error(e, __FILE__, __LINE__);
  return 0;
}

extern "C" int m2t_set_option(m2t_plan* p, const char* key, long long value) {
  if (!p || !key) return m2t_set_error(M2T_ERR_ARG, "m2t_set_option: null");
  const std::string k(key);
  if (k == "inference") {
    if (p->ws_initialised)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"inference\" makes or unmakes an inference plan only before the first m2t_plan_init_workspace");
    if (value == 0 && p->local_norm > 0)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"inference\" cannot be cleared while \"local_norm\" > 0 (local statistics exist on inference plans only: clear \"local_norm\" first)");
    if (value != 0 && p->health > 0)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"inference\" cannot be set while \"health\" > 0 (the health record exists on training plans only: clear \"health\" first)");
    p->inference = value != 0;
    p->have_acts = p->have_seed = p->l1_deferred = false;
    resolve_layout(p);
    return 0;
  }
  if (k == "local_norm") {
    if (value != 0 && (value < 8 || value > 16384)) return m2t_set_error(M2T_ERR_ARG, "local_norm: 0 (off) or 8 .. 16384 (the window side T)");
    if (p->ws_initialised)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"local_norm\" decides the workspace layout: it is set only before the first m2t_plan_init_workspace");
    if (!p->inference)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"local_norm\" needs an inference plan: set \"inference\" to 1 first (the backward pass has no local statistics)");
    p->local_norm = (int)value;
    resolve_layout(p);
    return 0;
  }
  if (k == "health") {
    if (value < 0 || value > 2) return m2t_set_error(M2T_ERR_ARG, "health: 0 (off), 1 (the forward's tensors) or 2 (and what the backward leaves)");
    if (p->ws_initialised)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"health\" decides the workspace layout: it is set only before the first m2t_plan_init_workspace");
    if (p->inference)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"health\" needs a training plan: this is an inference plan (option \"inference\"), which stores no stage");
    p->health = (int)value;
    resolve_layout(p);
    return 0;
  }
  if (k == "health_on") {
    if (value < 0 || value > 1) return m2t_set_error(M2T_ERR_ARG, "health_on: 0 / 1");
    if (p->inference)
      return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: \"health_on\" switches the health record of a training plan: this is an inference plan (option \"inference\")");
    p->health_on = (int)value;
    return 0;
  }
  if (p->health > 0 && p->ws_initialised && (k == "fused_tail" || k == "attn_bwd" || k == "fused_attn_fwd" || k == "fused_c16_fwd"))
    return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: this option decides which tensors are stored, and the rows of the health record (option \"health\") are fixed by m2t_plan_init_workspace: set it before");
  if (p->inference && p->ws_initialised)
    return m2t_set_error(M2T_ERR_STATE, "m2t_set_option: the layout of an initialised inference plan is frozen (set options before m2t_plan_init_workspace)");
  p->red_uploaded = false;     // the deferred-reduction table depends on the schedule: rebuild it on the next backward
  for (auto& kv : p->mask_tables) kv.second.uploaded = false;
  struct Resolve { m2t_plan* p; ~Resolve() { resolve_schedule(p); resolve_layout(p); } } resolve_on_return{p};     // whichever raw value changes below
  if (k == "side_stream") { p->use_side = (value != 0); return 0; }
  if (k == "fork_on_kernel") { p->fork_on_kernel = value != 0; return 0; }
  if (k == "fused_prep_fwd") { p->use_fused_prep_fwd = value != 0; return 0; }
  if (k == "fused_prep_bwd") { p->use_fused_prep_bwd = value != 0; return 0; }
  if (k == "fused_norm_red") { p->use_fused_norm_red = value != 0; return 0; }
  if (k == "fused_l1") { p->use_fused_l1 = value != 0; return 0; }
  if (k == "tail_bwd_mfma32") { p->use_tail_bwd32 = value != 0; return 0; }
  if (k == "fp32_fast") { p->use_fp32_fast = value != 0; return 0; }
  if (k == "fused_attn_fwd2") { if (value < -1 || value > 2) return m2t_set_error(M2T_ERR_ARG, "fused_attn_fwd2: -1 .. 2"); p->fused_attn_fwd2 = (int)value; return 0; }
  if (k == "gate_branch") { if (value < -1 || value > 3) return m2t_set_error(M2T_ERR_ARG, "gate_branch: -1..3"); p->gate_branch = (int)value; return 0; }
  if (k == "wgrad_big_tiles") { p->wgrad_big_tiles = (int)value; return 0; }
  if (k == "fused_tail") {
    if (value < 0 || value > 4) return m2t_set_error(M2T_ERR_ARG, "fused_tail: 0..4");
    p->use_fused_tail_bwd = value >= 1; p->use_fused_tail_fwd = value >= 2; p->use_stream_tail_fwd = value >= 3; p->use_stream_tail_bwd = value == 4;
    p->have_acts = false; return 0;
  }
  if (k == "attn_bwd") {
    if (value < 0 || value > 3) return m2t_set_error(M2T_ERR_ARG, "attn_bwd: 0..3");
    // (which of qkv1 / qkv2 the forward stores depends on this option: activations of a forward run under another value are unusable)
    p->use_resident_attn_bwd = value >= 1; p->use_fused_qkv_dgrad = value >= 2; p->use_c16_prep = value == 3; p->have_acts = false; return 0;
  }
  if (k == "conv_rows") { if (value < 0 || value > 1) return m2t_set_error(M2T_ERR_ARG, "conv_rows: 0 / 1"); p->use_conv_rows = (int)value; return 0; }
  if (k == "fused_conv_bwd") { p->use_fused_conv_bwd = (value != 0); return 0; }
  if (k == "fused_attn_fwd") { if (value < 0 || value > 2) return m2t_set_error(M2T_ERR_ARG, "fused_attn_fwd: 0..2"); p->use_fused_attn_fwd = (int)value; p->have_acts = false; return 0; }
  if (k == "fused_c16_fwd") { if (value < 0 || value > 2) return m2t_set_error(M2T_ERR_ARG, "fused_c16_fwd: 0..2"); p->use_fused_c16_fwd = (int)value; p->have_acts = false; return 0; }
  if (k == "debug_skip_side") { p->debug_skip_side = (value != 0); return 0; }
  return m2t_set_error(M2T_ERR_ARG, "m2t_set_option: unknown key");
}
extern "C" int m2t_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                             float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || n <= 0 || step < 1)
    return m2t_set_error(M2T_ERR_ARG, "m2t_adam_step: bad argument");
  return launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)stream);
}

extern "C" int m2t_grad_accumulate(float* acc, const float* g, long long n, float* loss_acc, const float* loss_part, void* stream) {
  if (n < 0 || (n > 0 && (!acc || !g)) || ((loss_acc == nullptr) != (loss_part == nullptr)))
    return m2t_set_error(M2T_ERR_ARG, "m2t_grad_accumulate: bad argument");
  return launch_grad_accumulate(acc, g, n, loss_acc, loss_part, (hipStream_t)stream);
}

extern "C" long long m2t_grad_norm_workspace_bytes(void) { return (long long)M2T_GNORM_BLOCKS * (long long)sizeof(double); }

extern "C" int m2t_grad_norm(const float* grads, long long n, float grad_scale, float max_norm, int skip_nonfinite, int step,
                             float beta1, float beta2, double* record, void* workspace, void* stream) {
  if (n < 0 || (n > 0 && !grads) || !record || !workspace || step < 1 || max_norm != max_norm)
    return m2t_set_error(M2T_ERR_ARG, "m2t_grad_norm: bad argument");
  return launch_grad_norm(grads, n, grad_scale, max_norm, skip_nonfinite != 0, step, beta1, beta2, record, (double*)workspace,
                          (hipStream_t)stream);
}

extern "C" int m2t_adam_step_ex(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                                float beta1, float beta2, float eps, int step, float grad_scale, float* ema, float weight_decay,
                                int decoupled, float ema_decay, const double* record, void* stream) {
  if (n < 0 || (n > 0 && (!params || !grads || !exp_avg || !exp_avg_sq)) || step < 1 || !(weight_decay >= 0.f) ||
      !(ema_decay >= 0.f && ema_decay < 1.f))
    return m2t_set_error(M2T_ERR_ARG, "m2t_adam_step_ex: bad argument");
  if (n == 0) return 0;
  return launch_adam_ex(params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, step, grad_scale, weight_decay,
                        decoupled != 0, ema_decay, record, (hipStream_t)stream);
}

// ---- stand-alone operators ---------------------------------------------------------------
extern "C" int m2t_dwt(int dtype, int levels, const void* src, void* dst, int B, int H, int W, int C, void* stream) {
  return launch_dwt(dtype, levels, src, C, 0, dst, C << (2 * levels), 0, B, H, W, C, false, (hipStream_t)stream);
}
extern "C" int m2t_iwt(int dtype, int levels, const void* src, void* dst, int B, int H, int W, int C, void* stream) {
  // src [B][H/S][W/S][C * 4^l] -> dst [B][H][W][C]
  return launch_dwt(dtype, levels, src, C << (2 * levels), 0, dst, C, 0, B, H, W, C, true, (hipStream_t)stream);
}
extern "C" int m2t_pixel_shuffle(const float* in, float* out, int B, int C, int H, int W, int r, void* stream) {
  return launch_pixel_shuffle_nchw(in, out, B, C, H, W, r, 0, (hipStream_t)stream);
}
extern "C" int m2t_pixel_unshuffle(const float* in, float* out, int B, int C, int H, int W, int r, void* stream) {
  // in [B][C][H*r][W*r] -> out [B][C*r*r][H][W]
  return launch_pixel_shuffle_nchw(in, out, B, C, H, W, r, 1, (hipStream_t)stream);
}
extern "C" int m2t_to_nhwc(int dtype, const float* nchw, void* nhwc, int B, int C, int HW, void* stream) {
  return launch_layout(dtype, nchw, nhwc, nullptr, B, C, HW, 0, (hipStream_t)stream);
}
extern "C" int m2t_to_nchw(int dtype, const void* nhwc, float* nchw, int B, int C, int HW, void* stream) {
  return launch_layout(dtype, nullptr, const_cast<void*>(nhwc), nchw, B, C, HW, 1, (hipStream_t)stream);
}
extern "C" int m2t_window_attention_fwd(int dtype, const void* qkv, const float* rel_h, const float* rel_w, void* out,
                                        int B, int h, int w, int C, void* stream) {
  return launch_window_attn_fwd(dtype, qkv, rel_h, rel_w, out, C, 0, nullptr, 0, B, h, w, C, (hipStream_t)stream);
}
extern "C" size_t m2t_window_attention_bwd_scratch_bytes(int dtype, int B, int h, int w, int C) {
  const size_t es = (dtype == M2T_F32) ? 4 : 2;
  const size_t nwin = (size_t)B * (h / 8) * (w / 8);
  return ((nwin * 100 * 2 * C * es + 255) & ~(size_t)255) + ((nwin * 10 * C * 4 + 255) & ~(size_t)255) + (size_t)32 * 10 * C * 4;
}
extern "C" int m2t_window_attention_bwd(int dtype, const void* qkv, const float* rel_h, const float* rel_w,
                                        const void* gout, void* gqkv, float* grel_h, float* grel_w, void* scratch, int B,
                                        int h, int w, int C, void* stream) {
  const size_t es = (dtype == M2T_F32) ? 4 : 2;
  const size_t nwin = (size_t)B * (h / 8) * (w / 8);
  const size_t woff = (nwin * 100 * 2 * C * es + 255) & ~(size_t)255;
  const size_t roff = woff + ((nwin * 10 * C * 4 + 255) & ~(size_t)255);
  int rc = launch_window_attn_bwd(dtype, qkv, rel_h, rel_w, gout, C, 0, gqkv, scratch, (float*)((char*)scratch + woff),
                                  B, h, w, C, (hipStream_t)stream, 0, true);
  if (rc) return rc;
  return launch_rel_reduce((float*)((char*)scratch + woff), (float*)((char*)scratch + roff), grel_h, grel_w, (int)nwin, C,
                           (hipStream_t)stream);
}
