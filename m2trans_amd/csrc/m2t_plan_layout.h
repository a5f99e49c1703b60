// m2t_plan_layout.h -- the workspace of an m2t_plan (m2t_api.hip), declared ONCE: m2t_plan_regions() enumerates every region with
// its name, handle slot, count, element type, class and its two schedule predicates; the training placement, the inference
// placement and the health record's rows are three readers of that enumeration.  m2t_resolve_workspace() rebuilds the name table
// and the workspace handles from it for the mode in force, every time an option changes.  Host code only: nothing here calls into
// a kernel file; the sizes kernels own come in as numbers (m2t_plan_geom) or through the declarations of m2t_kernels.h.
#pragma once
#include "m2t_kernels.h"
#include "m2t_layout.h"
#include "m2t_health_tile.h"
#include "../../include/m2t.h"

// ---- the resolved schedule ----------------------------------------------------------------------------------------------------
// Which kernel runs where, derived in ONE place (resolve_schedule of m2t_api.hip) from the raw option values m2t_set_option writes,
// the element type, the scale and the shape.  m2t_forward, the backward pass, m2t_plan_query and the region predicates below read
// these fields and never combine raw options themselves: a new option is resolved there and nowhere else.  Per-pass conditions
// (stage masks, debug_skip_side, stream capture, red_uploaded, l1_deferred) stay with the pass and combine with these fields.
enum m2t_tail_fwd { TAIL_FWD_PLAIN, TAIL_FWD_TILE, TAIL_FWD_STREAM, TAIL_FWD_X23_STREAM };
enum m2t_tail_bwd { TAIL_BWD_PLAIN, TAIL_BWD_STORED, TAIL_BWD_RC16, TAIL_BWD_RC32, TAIL_BWD_STREAM, TAIL_BWD_X23_STREAM };
struct m2t_sched {
  // forward attention (bf16 only)
  bool c16_fused_fwd;      // C = 16: norm apply + qkv projection + attention + residual in one kernel (k_attn_c16.hip)
  bool c16_recompute;      // ... and qkv1 is not stored: the wave-per-window backward recomputes it from d1
  bool c64_fused_fwd;      // C >= 64: qkv projection + attention + epilogue in one kernel (k_attn_fused.hip)
  bool prep_in_fwd;        // ... with branch_prep inside
  bool c64_recompute;      // qkv2 (C = 64) is not stored: the resident backward recomputes it from d2
  int fwd2;                // C = 256 with branch_prep inside: variant of the two-windows-per-CU kernels (k_attn_fwd2.hip), 0 = not used
  // backward attention (bf16 only)
  bool resident_bwd;       // whole-window-resident attention backward (k_attn_res.hip)
  bool fused_dgrad;        // C >= 64: projection data gradient inside that kernel
  bool c16_prep;           // C = 16: overlap-add + projection data gradient + branch_prep_bwd in one kernel
  bool prep_in_bwd;        // branch 4's branch_prep_bwd inside branch 3's attention backward
  bool norm_red_in_prep;   // first stage of the InstanceNorm backward reduction inside the C = 16 prep launch
  // tail
  m2t_tail_fwd tail_fwd;
  m2t_tail_bwd tail_bwd;
  bool l1_in_tail;         // a deferred L1 loss is taken inside the fused tail backward (else by m2t_l1_loss's kernel)
  // feed-forward conv
  bool conv_rows;          // bf16: the row-streaming LDS-DMA kernel
  int conv_variant;        // the launchers' variant argument: 0 = row-streaming where the element type has it, 1 = tile
  bool fused_conv_bwd;     // bf16: data + weight / bias gradient in one row-streaming pass
  // weight packs of the C >= 64 qkv weights the forward must refresh: plain copies (unfused forward GEMM), transposes (unfused dgrad GEMM)
  bool need_copy, need_tr;
  // what the forward leaves in the workspace
  bool stores_qkv1, stores_qkv2, stores_t1, stores_t2;
  bool fork_on_kernel;     // fork events ride on the dispatch they follow (needs the side stream; not under stream capture)
};

static const int BR_C[4] = {16, 64, 256, 256};
static const int BR_L[4] = {0, 1, 2, 2};

// ---- handles: names resolved to plain offsets; the passes index these structs and look nothing up -------------------------------
// Workspace offsets (bytes) are rebuilt by m2t_resolve_workspace() after every change of an option: a region the mode and schedule
// in force do not place is ABSENT: its handle is M2T_NO_REGION, which is what every workspace handle starts as; its name is not in
// the table (m2t_plan_query answers -1) and the kernel that would write it gets a null pointer.  Parameter offsets (floats) and
// pack offsets (elements) are set once, by m2t_plan_create, and never touched again: they live in the derived part of the two
// structs, which m2t_clear_workspace_handles() leaves alone, so the passes spell bh.mean and bh.wqkv[i] alike.
static const size_t M2T_NO_REGION = ~(size_t)0;
static inline char* region_ptr(char* ws, size_t off) { return off == M2T_NO_REGION ? nullptr : ws + off; }
#define M2T_NR4 {M2T_NO_REGION, M2T_NO_REGION, M2T_NO_REGION, M2T_NO_REGION}
struct m2t_block_ws {
  size_t mean = M2T_NO_REGION, rstd = M2T_NO_REGION, xc = M2T_NO_REGION, d[4] = M2T_NR4, qkv[4] = M2T_NR4;
};
struct m2t_block_handles : m2t_block_ws {
  long long rel_h[4], rel_w[4], wqkv[4], ffw, ffb;                          // parameters
  long long w[4], wT[4], wF[4], wTF[4], wf, wfT, wfR, wfTR;                 // packs (wF / wTF: C >= 64 only)
};
struct m2t_plan_ws {
  std::vector<size_t> X;                                                    // nb + 1 feature maps: block b reads X[b], writes X[b + 1]
  size_t zero_page = M2T_NO_REGION, pack_descs = M2T_NO_REGION, pack_blocks = M2T_NO_REGION, packed = M2T_NO_REGION,
         xin = M2T_NO_REGION, norm_part = M2T_NO_REGION, norm_s = M2T_NO_REGION, vring = M2T_NO_REGION, norm_part0 = M2T_NO_REGION,
         t1act = M2T_NO_REGION, t1der = M2T_NO_REGION, t2act = M2T_NO_REGION, t2der = M2T_NO_REGION, srpre = M2T_NO_REGION,
         loss_part = M2T_NO_REGION, gpre = M2T_NO_REGION, g_t2pre = M2T_NO_REGION, g_t1pre = M2T_NO_REGION, gT = M2T_NO_REGION,
         gA = M2T_NO_REGION, gB = M2T_NO_REGION, gxc = M2T_NO_REGION, gn = M2T_NO_REGION, gd = M2T_NO_REGION, gd2 = M2T_NO_REGION,
         gdwin = M2T_NO_REGION, gdwin2 = M2T_NO_REGION, head_cols = M2T_NO_REGION, gqkv[2][4] = {M2T_NR4, M2T_NR4},
         win[2][4] = {M2T_NR4, M2T_NR4}, relw[2][4] = {M2T_NR4, M2T_NR4}, arena = M2T_NO_REGION, red_descs = M2T_NO_REGION;
  size_t xn = M2T_NO_REGION, lnsum = M2T_NO_REGION, norm_id = M2T_NO_REGION;            // option "local_norm"
  size_t health = M2T_NO_REGION, health_part = M2T_NO_REGION, health_descs = M2T_NO_REGION, health_work = M2T_NO_REGION;   // option "health"
};
struct m2t_plan_handles : m2t_plan_ws {
  std::vector<m2t_block_handles> blk;
  long long head_w, head_b, tail0_w, tail0_b, tail3_w, tail3_b, wlast;      // parameters (wlast: the tail conv; tail3_*: x4 only)
  long long t0, t0T, t3, t3T;                                               // packs (t3 / t3T: x4 only)
};
// every workspace handle absent; hd.blk keeps its nb entries and their parameter and pack offsets
static inline void m2t_clear_workspace_handles(m2t_plan_handles& hd) {
  static_cast<m2t_plan_ws&>(hd) = m2t_plan_ws{};
  hd.X.assign(hd.blk.size() + 1, M2T_NO_REGION);
  for (m2t_block_handles& bh : hd.blk) static_cast<m2t_block_ws&>(bh) = m2t_block_ws{};
}

// ---- what the counts are made of: the plan's shape, its layout-deciding options, and the sizes other code owns -------------------
struct m2t_plan_geom {
  int B, H0, W0, H, W, scale, nb, dt;
  size_t esz;
  long long P;                       // padded LR pixels per image
  int Hs, Ws, Hsp, Wsp;              // SR size (cropped) and padded SR size
  // option "inference": m2t_forward alone, on a forward-only workspace (the inference placement below)
  int inference = 0;
  // option "local_norm" (inference plans only): T > 0 = every block normalises with the statistics of a T x T window around each pixel
  // (k_local_norm.hip -> region "xn") and its unchanged consumers get xn with the identity record "norm_id" (mean 0, rstd 1)
  int local_norm = 0;
  // option "health" (training plans only): 1 = a record of the tensors the forward stores, 2 = and of what the backward leaves
  // (k_health.hip)
  int health = 0;
  // set by m2t_plan_create: pack descriptors, ints of the pack work list, packed elements, parameters (floats), elements of the
  // ring buffer of k_attn_fwd2.hip (window_attn_fwd2_vring_elems), floats of the slab arena
  size_t n_pack_descs = 0, n_pack_block_ints = 0, npacked = 0, nparams = 0, vring_elems = 0, arena_floats = 0;
};

// ---- the declarations ------------------------------------------------------------------------------------------------------------
enum m2t_elem { M2T_EL_T, M2T_EL_F32, M2T_EL_F64, M2T_EL_BYTE };       // the plan's element type, always fp32, fp64, bytes
enum m2t_region_class {
  M2T_RC_PERSISTENT,     // tables m2t_plan_init_workspace fills and the packed weights: every plan has them
  M2T_RC_FORWARD,        // written by m2t_forward
  M2T_RC_BACKWARD,       // written by the loss and the backward pass alone: no inference plan has them
  M2T_RC_LOCAL_NORM,     // option "local_norm": inference plans with T > 0 only
  M2T_RC_HEALTH          // option "health": training plans with a level > 0 only, behind the training layout
};
struct m2t_region_decl {
  std::string name;
  size_t* slot;          // the handle it fills, in the handle set given to m2t_plan_regions; nullptr: a name without a handle
  size_t n, es;          // element count, bytes per element
  m2t_elem el;
  int block;             // k of a "b<k>." region, b of "X<b>", else -1
  m2t_region_class cls;
  bool fwd_reads;        // m2t_forward reads it under the schedule: an inference plan places it
  bool whole;            // a pass writes all of it under the schedule: the health record may have a row for it
};
// the health record's rows (option "health"), resolved from the declarations: the passes use the descriptor table, the work list
// and the counts and look nothing up
struct m2t_health_table {
  std::vector<std::string> names;              // row -> name ("sr", a "ws:" name, "grads")
  std::vector<m2t_health_desc> descs;
  std::vector<int> work;                       // (row, chunk) pairs, forward rows first
  std::vector<int> decl;                       // row -> index of its declaration, -1 for the two buffers a pass gets from its caller
  int rows_fwd = 0, items_fwd = 0;
};
struct m2t_plan_table {
  std::vector<m2t_region_decl> regions;        // in the training layout's order
  m2t_health_table health;                     // offsets not yet set (m2t_health_rows)
};

// Does m2t_forward need the region d<i + 1> / qkv<i + 1> under schedule s?  (A training plan stores both for the backward pass whatever
// this says.)
static bool forward_reads_d(const m2t_sched& s, int i) {
  if (i == 0) return !s.c16_fused_fwd;                       // the fused C = 16 kernel normalises in registers: d1 is "for the backward"
  if (!s.prep_in_fwd) return true;                           // branch_prep writes d, the projection reads it
  // branch_prep inside the fused kernel: nothing reads d in the forward.  The C = 64 kernel has an instantiation without the store; the
  // C = 256 kernels keep it (k_attn_fused.hip: at 256 VGPRs the kernel spills without it; k_attn_fwd2.hip takes no null), and so their region
  return BR_C[i] == 256;
}
static bool forward_reads_qkv(const m2t_sched& s, int i) {
  if (i == 0) return !s.c16_fused_fwd;
  if (!s.c64_fused_fwd) return true;                         // projection GEMM -> attention kernel
  return BR_C[i] == 256 && s.prep_in_fwd && s.fwd2 != 0;     // k_attn_fwd2.hip re-reads the window's own v rows from the qkv tensor
}

// The health record's rows, from the declarations made so far and the schedule behind their `whole` flags.  A tensor the schedule
// does not store (q | k | v on the recomputing attention paths, the tail's GELU tensors on the fused tails) has no row; neither has a
// scratch region a pass only partly writes (xin, the ring buffers, the slab arena).  The order is part of the query surface
// ("health_row:", "health_name:<i>"), so it is walked out here and not taken from the declarations': sr, the forward's regions in
// the order m2t_forward writes them, then at level 2 the backward's in the order it writes them, then grads.
static void m2t_health_walk(const m2t_plan_geom& g, m2t_plan_table& tb) {
  m2t_health_table& ht = tb.health;
  std::map<std::string, int> index;            // name -> position in regions
  for (size_t i = 0; i < tb.regions.size(); ++i) index[tb.regions[i].name] = (int)i;
  auto row = [&](const std::string& name, int phase, long long ext_n) {
    m2t_health_desc d{};
    d.phase = phase;
    int di = -1;
    if (ext_n >= 0) { d.off = -1; d.n = ext_n; d.dtype = M2T_F32; }
    else {
      auto it = index.find(name);
      if (it == index.end() || !tb.regions[it->second].whole) return;
      const m2t_region_decl& r = tb.regions[di = it->second];
      d.n = (long long)r.n; d.dtype = r.el == M2T_EL_F32 ? M2T_F32 : g.dt;
    }
    d.item0 = (int)(ht.work.size() / 2);
    d.nitems = (int)std::max<long long>(1, ceil_divll(d.n, health_tile::CHUNK));
    for (int c = 0; c < d.nitems; ++c) { ht.work.push_back((int)ht.descs.size()); ht.work.push_back(c); }
    ht.names.push_back(name);
    ht.descs.push_back(d);
    ht.decl.push_back(di);
  };
  auto ws_row = [&](const std::string& name, int phase) { row(name, phase, -1); };
  row("sr", 0, (long long)g.B * 3 * g.Hs * g.Ws);
  ws_row("X0", 0);
  for (int b = 0; b < g.nb; ++b) {
    const std::string k = "b" + std::to_string(b) + ".";
    ws_row(k + "mean", 0); ws_row(k + "rstd", 0);
    for (int i = 0; i < 4; ++i) { ws_row(k + "d" + std::to_string(i + 1), 0); ws_row(k + "qkv" + std::to_string(i + 1), 0); }
    ws_row(k + "xc", 0);
    ws_row("X" + std::to_string(b + 1), 0);
  }
  for (const char* n : {"t1act", "t1der", "t2act", "t2der", "srpre"}) ws_row(n, 0);
  ht.rows_fwd = (int)ht.descs.size();
  ht.items_fwd = (int)(ht.work.size() / 2);
  if (g.health >= 2) {
    for (const char* n : {"g_t2pre", "g_t1pre", "gT", "gA", "gB"}) ws_row(n, 1);
    for (int set = 0; set < 2; ++set)                               // dq | dK | dV of the last block that used the buffer set
      for (int i = 0; i < 4; ++i) ws_row("gqkv" + std::to_string(i) + (set ? "b" : ""), 1);
    ws_row("gn", 1);
    ws_row("gxc", 1);                                               // after block 0: g(res), the head's cotangent
    row("grads", 1, (long long)g.nparams);
  }
}

// Every region of the plan's workspace, once, in the order of the training layout.  `hd` is the handle set the slots point into.
static m2t_plan_table m2t_plan_regions(const m2t_plan_geom& g, const m2t_sched& s, m2t_plan_handles& hd) {
  m2t_plan_table tb;
  const int B = g.B, sc = g.scale, r0 = (sc == 4) ? 2 : sc, nb = g.nb;
  const bool x4 = sc == 4;
  const long long BP = (long long)B * g.P;
  const m2t_elem T = M2T_EL_T, F32 = M2T_EL_F32, F64 = M2T_EL_F64, BYTE = M2T_EL_BYTE;
  const m2t_region_class PERSISTENT = M2T_RC_PERSISTENT, FORWARD = M2T_RC_FORWARD, BACKWARD = M2T_RC_BACKWARD,
                         LOCAL_NORM = M2T_RC_LOCAL_NORM, HEALTH = M2T_RC_HEALTH;
  auto add = [&](const std::string& name, size_t* slot, size_t n, m2t_elem el, m2t_region_class cls, bool fwd_reads, bool whole = false,
                 int block = -1) {
    const size_t es = el == T ? g.esz : (el == F32 ? 4 : (el == F64 ? 8 : 1));
    tb.regions.push_back(m2t_region_decl{name, slot, n, es, el, block, cls, fwd_reads, whole});
  };
  // the counts more than one region has
  const size_t n_map = BP * 64, n_quarter = BP * 16, n_qkv = BP * 48;       // a 64-channel feature map, one branch's 16 of them, its q | k | v
  const size_t n_stat = B * 64;                                             // one value per (image, channel)
  const size_t n_t1 = BP * r0 * r0 * 64, n_t2 = BP * 16 * 64;               // the tail's first / second expansion
  const size_t n_sr = (size_t)B * 3 * g.Hsp * g.Wsp;                        // the padded SR image
  add("zero_page", &hd.zero_page, 256, BYTE, PERSISTENT, true);          // source of every out-of-image pixel the LDS-DMA kernels stage (k_conv.hip)
  add("pack_descs", &hd.pack_descs, g.n_pack_descs * sizeof(m2t_pack_desc), BYTE, PERSISTENT, true);
  add("pack_blocks", &hd.pack_blocks, g.n_pack_block_ints * sizeof(int), BYTE, PERSISTENT, true);
  add("packed", &hd.packed, g.npacked, T, PERSISTENT, true);
  for (int b = 0; b <= nb; ++b) add("X" + std::to_string(b), &hd.X[b], n_map, T, FORWARD, true, true, b);
  for (int b = 0; b < nb; ++b) {
    m2t_block_handles& bh = hd.blk[b];
    const std::string k = "b" + std::to_string(b) + ".";
    add(k + "mean", &bh.mean, n_stat, F32, FORWARD, true, true, b);
    add(k + "rstd", &bh.rstd, n_stat, F32, FORWARD, true, true, b);
    add(k + "xc", &bh.xc, n_map, T, FORWARD, true, true, b);
    for (int i = 0; i < 4; ++i) {
      add(k + "d" + std::to_string(i + 1), &bh.d[i], n_quarter, T, FORWARD, forward_reads_d(s, i), true, b);
      add(k + "qkv" + std::to_string(i + 1), &bh.qkv[i], n_qkv, T, FORWARD, forward_reads_qkv(s, i),
          i == 0 ? s.stores_qkv1 : (i == 1 ? s.stores_qkv2 : true), b);
    }
  }
  add("xin", &hd.xin, n_quarter, T, FORWARD, true);
  // "a", "ga", "rel_part" and "col_part" have a name and no handle: no pass reads them.  They keep their sizes and places because
  // every later offset would move without them
  add("a", nullptr, n_quarter, T, FORWARD, false);
  add("norm_part", &hd.norm_part, (size_t)B * 8 * M2T_NORM_SPLIT * 64 * 3, F32, FORWARD, true);      // (the conv epilogue leaves up to 256 partials per image)
  add("norm_s", &hd.norm_s, n_stat * 2, F32, BACKWARD, false);
  add("vring", &hd.vring, g.vring_elems, T, FORWARD, s.fwd2 != 0);          // v rows of the ring keys (k_attn_fwd2.hip)
  add("norm_part0", &hd.norm_part0, (size_t)B * g.H * (g.W / 16) * 32, F32, BACKWARD, false);      // per-tile plane-0 partials of the InstanceNorm backward (fused_norm_red)
  // tail activations: gelu(t) and gelu'(t) of each expansion (the pre-activation t itself is never needed again)
  add("t1act", &hd.t1act, n_t1, T, FORWARD, s.stores_t1, s.stores_t1);
  // gelu'(t1): read by the backward pass alone.  fp32 x3 keeps it: that expansion runs on the generic GEMM, whose epilogue always stores it
  add("t1der", &hd.t1der, n_t1, T, FORWARD, g.dt == M2T_F32 && sc == 3, s.stores_t1);
  if (x4) {
    add("t2act", &hd.t2act, n_t2, T, FORWARD, s.stores_t2, s.stores_t2);
    add("t2der", &hd.t2der, n_t2, T, FORWARD, false, s.stores_t2);
  }
  add("srpre", &hd.srpre, n_sr, F32, FORWARD, true, true);
  add("loss_part", &hd.loss_part, M2T_LOSS_BLOCKS, F32, BACKWARD, false);
  // backward
  add("gpre", &hd.gpre, n_sr, F32, BACKWARD, false);
  if (x4) add("g_t2pre", &hd.g_t2pre, n_t2, T, BACKWARD, false, s.tail_bwd == TAIL_BWD_PLAIN);
  add("g_t1pre", &hd.g_t1pre, n_t1, T, BACKWARD, false, s.tail_bwd != TAIL_BWD_X23_STREAM);
  add("gT", &hd.gT, n_map, T, BACKWARD, false, true);
  add("gA", &hd.gA, n_map, T, BACKWARD, false, nb >= 3);                    // g(X<b>) of the even / odd blocks b >= 1
  add("gB", &hd.gB, n_map, T, BACKWARD, false, nb >= 2);
  add("gxc", &hd.gxc, n_map, T, BACKWARD, false, true);
  add("gn", &hd.gn, n_map, T, BACKWARD, false, true);
  add("ga", nullptr, n_quarter, T, BACKWARD, false);
  add("gd", &hd.gd, n_quarter, T, BACKWARD, false);
  add("gd2", &hd.gd2, n_quarter, T, BACKWARD, false);      // second set: a branch's attention backward reads the previous branch's rows while it writes its own (fused_prep_bwd)
  add("gdwin2", &hd.gdwin2, BP * 9, T, BACKWARD, false);
  add("gdwin", &hd.gdwin, BP * 9, T, BACKWARD, false);      // ring rows of the fused projection data gradient: [windows][36][C], windows * C = BP / 4
  add("head_cols", &hd.head_cols, BP * 32, T, BACKWARD, false);
  for (int i = 0; i < 4; ++i) {     // TWO sets per branch (even / odd blocks): the side stream may lag the main chain by two blocks, and
    for (int set = 0; set < 2; ++set) {   // the main chain waits for it once per block instead of once per branch
      const std::string sfx = std::to_string(i) + (set ? "b" : "");
      add("gqkv" + sfx, &hd.gqkv[set][i], n_qkv, T, BACKWARD, false, set == 0 || nb >= 2);
      add("win" + sfx, &hd.win[set][i], BP * 50, T, BACKWARD, false);
      add("relw" + sfx, &hd.relw[set][i], (size_t)(BP / 64) * 10 * 16, F32, BACKWARD, false);
    }
  }
  add("rel_part", nullptr, 32 * 10 * 256, F32, BACKWARD, false);
  add("arena", &hd.arena, g.arena_floats, F32, BACKWARD, false);      // every slab set of one backward pass (see m2t_backward)
  add("red_descs", &hd.red_descs, 512 * sizeof(m2t_red_desc), BYTE, BACKWARD, false);
  add("col_part", nullptr, (size_t)256 * 768, F32, BACKWARD, false);
  // local_norm: the normalised block input (one buffer for every block: a block's consumers are done with it before the next block's
  // statistics run), the fp64 {sum x, sum x^2} pairs between its two passes, and the identity record [mean = 0 | rstd = 1], [B][64] each
  const bool ln = g.local_norm > 0;
  add("xn", &hd.xn, n_map, T, LOCAL_NORM, ln);
  add("lnsum", &hd.lnsum, n_map * 2, F64, LOCAL_NORM, ln);
  add("norm_id", &hd.norm_id, n_stat * 2, F32, LOCAL_NORM, ln);
  // the health record: descriptor table and work list next to the other tables, the record (a header row and one per row), the
  // per-chunk partials
  if (g.health > 0) m2t_health_walk(g, tb);
  const size_t rows = tb.health.descs.size(), items = tb.health.work.size() / 2;
  add("health_descs", &hd.health_descs, rows * sizeof(m2t_health_desc), BYTE, HEALTH, false);
  add("health_work", &hd.health_work, items * 2 * sizeof(int), BYTE, HEALTH, false);
  add("health", &hd.health, (1 + rows) * health_tile::SLOTS, F64, HEALTH, false);
  add("health_part", &hd.health_part, items * health_tile::SLOTS, F64, HEALTH, false);
  return tb;
}

// ---- the three readers -----------------------------------------------------------------------------------------------------------
static inline void m2t_place(const m2t_region_decl& d, m2t_region& ws) {
  const size_t off = ws.add(d.name, d.n, d.es);
  if (d.slot) *d.slot = off;
}
// training: every region of the persistent, forward and backward classes, in declaration order
static void m2t_place_training(const m2t_plan_table& tb, m2t_region& ws) {
  for (const m2t_region_decl& d : tb.regions)
    if (d.cls <= M2T_RC_BACKWARD) m2t_place(d, ws);
}
// inference: the regions the forward reads (the local-norm regions among them when the option is on).  Two rules of this placement:
// ONE set of per-block regions under every "b<k>." name, and X1 .. X<nb> alternate between two buffers (block b reads X<b> and
// writes X<b + 1>; the last block's conv adds X0), so X<b>, b >= 3, is X<b - 2>.  An aliased name answers ws: / wsn: like its target
static void m2t_place_inference(const m2t_plan_table& tb, m2t_region& ws) {
  for (const m2t_region_decl& d : tb.regions) {
    if (!d.fwd_reads) continue;
    const size_t dot = d.name.find('.');                     // "b<k>.<what>" or "X<b>"
    const bool per_block = d.block >= 0 && dot != std::string::npos;
    if (d.block < 0 || d.block <= (per_block ? 0 : 2)) { m2t_place(d, ws); continue; }
    auto of = ws.t.find(per_block ? "b0" + d.name.substr(dot) : "X" + std::to_string(d.block - 2));
    ws.t[d.name] = of->second;
    *d.slot = of->second.off;
  }
}
// the health record's four regions, behind the training layout
static void m2t_place_health(const m2t_plan_table& tb, m2t_region& ws) {
  for (const m2t_region_decl& d : tb.regions)
    if (d.cls == M2T_RC_HEALTH) m2t_place(d, ws);
}
// the health rows once their regions are placed: a row's offset is its declaration's handle
static m2t_health_table m2t_health_rows(const m2t_plan_table& tb) {
  m2t_health_table ht = tb.health;
  for (size_t r = 0; r < ht.descs.size(); ++r)
    if (ht.decl[r] >= 0) ht.descs[r].off = (long long)*tb.regions[ht.decl[r]].slot;
  return ht;
}

// the name table, the workspace handles and the health rows that go with g (its mode and options) and the schedule s
static void m2t_resolve_workspace(const m2t_plan_geom& g, const m2t_sched& s, m2t_plan_handles& hd, m2t_region& ws, m2t_health_table& ht) {
  m2t_clear_workspace_handles(hd);
  ws.clear();
  const m2t_plan_table tb = m2t_plan_regions(g, s, hd);
  if (g.inference) m2t_place_inference(tb, ws);
  else {
    m2t_place_training(tb, ws);
    if (g.health > 0) m2t_place_health(tb, ws);
  }
  ws.seal();
  ht = m2t_health_rows(tb);
}
