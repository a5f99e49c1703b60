// m2t_rlutrans_layout.h -- the flat parameter vector of TransBlock(n_feat=64, dim=64) and the training workspace, shared by
// m2t_rlutrans.hip (host layer) and k_rlutrans_bwd.hip (backward kernels).
#pragma once
#include <cstddef>

constexpr int TB_DIM = 64, TB_HEADS = 8, TB_HD = 8, TB_HID = 16;
// flat parameter buffer = state_dict order of TransBlock(n_feat=64, dim=64)
constexpr long long OFF_REDUCE = 0, OFF_QKV = OFF_REDUCE + 64 * 64, OFF_PROJ_W = OFF_QKV + 192 * 64, OFF_PROJ_B = OFF_PROJ_W + 64 * 64,
                    OFF_N1W = OFF_PROJ_B + 64, OFF_N1B = OFF_N1W + 64, OFF_FC1W = OFF_N1B + 64, OFF_FC1B = OFF_FC1W + 16 * 64,
                    OFF_FC2W = OFF_FC1B + 16, OFF_FC2B = OFF_FC2W + 64 * 16, OFF_N2W = OFF_FC2B + 64, OFF_N2B = OFF_N2W + 64,
                    TB_NPARAMS = OFF_N2B + 64;
static_assert(TB_NPARAMS == 22928, "parameter count of TransBlock(dim=64) (SURVEY A17)");
// the transposed weights of the data-gradient GEMMs, behind the 22 928 packed values (elements)
constexpr long long OFF_FC1T = TB_NPARAMS, OFF_PROJT = OFF_FC1T + 64 * 16, OFF_QKVT = OFF_PROJT + 64 * 64, OFF_REDUCET = OFF_QKVT + 64 * 192,
                    TB_NPACKED = OFF_REDUCET + 64 * 64;

#define TB_COLSUM_BLOCKS 256     // partial rows of a bias / LayerNorm-affine column sum (first stage)
#define TB_MAX_SLABS 512         // upper bound of the slabs one weight gradient leaves (wgrad_slab_count never exceeds it here)
// slabs / partial rows this many tokens can leave (launch_wgrad_tn: one slab per 128 rows at most; launch_colsum: one block per 64)
inline size_t tb_max_slabs(long long M) { const long long n = (M + 127) / 128; return (size_t)(n < TB_MAX_SLABS ? n : TB_MAX_SLABS); }
inline size_t tb_max_colsum_blocks(long long M) { const long long n = (M + 63) / 64; return (size_t)(n < TB_COLSUM_BLOCKS ? n : TB_COLSUM_BLOCKS); }

enum tb_train_region { TB_R_H1 = 0, TB_R_AO, TB_R_WTS, TB_R_X, TB_R_HN1, TB_R_R, TB_R_QKV, TB_R_X1, TB_R_HN2, TB_R_COUNT };

// Training workspace: [saved by forward_train | scratch of the backward].  es = bytes of the compute element type.
struct TbTrainLayout {
  size_t es, wts, X, Hn1, R, QKV, AO, X1, Hn2, H1, Y;                 // saved (Y: the block output before its fp32 copy)
  size_t gyT, gH1, gA, gB, gX1f, gX1t, gQKV, stats, arena, total;     // scratch
  // arena (floats): weight-gradient slabs, then the column-sum partials
  size_t a_wr, a_wqkv, a_wp, a_w1, a_w2, a_bp, a_b1, a_b2, a_ln1, a_ln2, arena_floats;
  TbTrainLayout(long long M, int f32) {
    es = f32 ? 4 : 2;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    auto take = [&](size_t& field, size_t bytes) { field = o; o += al(bytes); };
    const size_t m = (size_t)M;
    take(wts, (size_t)TB_NPACKED * es);
    take(X, m * 64 * es); take(Hn1, m * 64 * es); take(R, m * 64 * es); take(QKV, m * 192 * es); take(AO, m * 64 * es);
    take(X1, m * 64 * es); take(Hn2, m * 64 * es); take(H1, m * 16 * es); take(Y, m * 64 * es);
    take(gyT, m * 64 * es); take(gH1, m * 16 * es); take(gA, m * 64 * es); take(gB, m * 64 * es);
    take(gX1f, m * 64 * 4); take(gX1t, m * 64 * es); take(gQKV, m * 192 * es);
    take(stats, m * TB_HEADS * 3 * 4);                                 // per (token, head): softmax maximum, 1 / sum, delta
    size_t a = 0;
    const size_t ns = tb_max_slabs(M), nc = tb_max_colsum_blocks(M);
    auto atake = [&](size_t& field, size_t n) { field = a; a += (n + 63) & ~(size_t)63; };
    atake(a_wr, ns * 64 * 64); atake(a_wqkv, ns * 192 * 64); atake(a_wp, ns * 64 * 64);
    atake(a_w1, ns * 16 * 64); atake(a_w2, ns * 64 * 16);
    atake(a_bp, nc * 64); atake(a_b1, nc * 16); atake(a_b2, nc * 64);
    atake(a_ln1, nc * 128); atake(a_ln2, nc * 128);
    arena_floats = a;
    take(arena, a * 4);
    total = o;
  }
};
