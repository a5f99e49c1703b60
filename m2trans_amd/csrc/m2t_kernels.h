// m2t_kernels.h -- internal launcher prototypes shared by the .hip files and the C-ABI layer.
#pragma once
#include <algorithm>
#include "m2t_common.h"
#include "m2t_pixel_loss.h"
#include <hip/hip_ext.h>

#define M2T_NORM_SPLIT 32     // pixel splits per image in the InstanceNorm reductions
#define M2T_LOSS_BLOCKS 1024  // partial sums of the L1 loss
#define M2T_MAX_SLABS 1024    // split-M slabs of a weight-gradient GEMM
#define M2T_UNSUPPORTED (-1000)
#define M2T_PACK_CHUNK 2048   // output elements one workgroup of the weight-packing kernel converts

enum m2t_pack_kind {
  M2T_PACK_COPY = 0, M2T_PACK_TRANSPOSE = 1, M2T_PACK_CONV3 = 2, M2T_PACK_CONV3_T = 3,
  M2T_PACK_SHUF_ROWS = 4, M2T_PACK_SHUF_ROWS_T = 5,
  M2T_PACK_FRAG16 = 6,    // src [N = d0][K = d1] -> MFMA A-operand fragment order [N/16][K/32][64 lanes][8]: element j of lane l of
                          // fragment (tile, ks) is src[16 tile + (l & 15)][32 ks + 8 (l >> 4) + j]; one wave load = 1 KB contiguous
  M2T_PACK_FRAG16_T = 7,  // the same fragments of the TRANSPOSE: src is [K = d1][N = d0] (element = src[32 ks + 8 (l >> 4) + j][16 tile + (l & 15)])
  M2T_PACK_CONV3_ROWS = 8,    // 64 -> 64 3x3 conv weight as the register-resident A-fragments of conv3x3_c64_rows_kernel:
  M2T_PACK_CONV3_ROWS_T = 9   // [tap][channel half][k-chunk][tile][64 lanes][8], one contiguous 1 KB per wave load (_T: data gradient)
};
struct m2t_red_desc {      // one deferred slab reduction: grads[dst_off + perm(e)] = sum_s arena[src_off + s*n + e]
  long long src_off, dst_off, n;
  int ns, perm, p0, p1, p2, pad_;
};
struct m2t_pack_desc {
  long long src_off, dst_off, n;
  int kind, d0, d1, d2;
};

// ---- in-library kernel timing (HIP events on the launch stream; off by default) -----------
enum m2t_prof_cat {
  M2T_PROF_ATTN_FWD_16 = 0, M2T_PROF_ATTN_FWD_64, M2T_PROF_ATTN_FWD_256,
  M2T_PROF_ATTN_BWD_16, M2T_PROF_ATTN_BWD_64, M2T_PROF_ATTN_BWD_256,
  M2T_PROF_CONV3_FWD, M2T_PROF_CONV3_DGRAD, M2T_PROF_CONV3_WGRAD,
  M2T_PROF_GEMM_QKV, M2T_PROF_GEMM_QKV_DGRAD, M2T_PROF_WGRAD_QKV,
  M2T_PROF_TAIL_GEMM, M2T_PROF_TAIL_WGRAD, M2T_PROF_FINAL_FWD, M2T_PROF_FINAL_DGRAD, M2T_PROF_FINAL_WGRAD,
  M2T_PROF_ATTN_FUSED_64, M2T_PROF_ATTN_FUSED_256,      // fused qkv projection + window attention forward (k_attn_fused.hip)
  M2T_PROF_TAIL_FWD_FUSED,                              // tail.3 expansion + PixelShuffle + GELU + tail conv (k_tail_fwd.hip)
  M2T_PROF_ATTN_FUSED_16,                               // InstanceNorm apply + qkv projection + window attention, C = 16 (k_attn_c16.hip)
  M2T_PROF_CONV3_BWD,                                   // conv 64 -> 64 data + weight gradient in one pass (k_conv.hip)
  M2T_PROF_NCAT
};
void m2t_prof_begin(int cat, hipStream_t st);
void m2t_prof_end(int cat, hipStream_t st);
// Single-kernel categories (attention, conv3x3, final conv): the scope's two events ride on the kernel dispatch itself
// (hipExtLaunchKernelGGL start / stop events = the dispatch's own begin / end timestamps, the quantity rocprofv3
// reports) instead of bracketing it with marker packets, which add the ~5 us launch gap to every sample.
#define M2T_PROF_DISPATCH_CATS ((1ull << M2T_PROF_GEMM_QKV) - 1ull | (1ull << M2T_PROF_FINAL_FWD) | (1ull << M2T_PROF_FINAL_DGRAD) | (1ull << M2T_PROF_FINAL_WGRAD) | \
                                (1ull << M2T_PROF_ATTN_FUSED_64) | (1ull << M2T_PROF_ATTN_FUSED_256) | (1ull << M2T_PROF_TAIL_FWD_FUSED) | (1ull << M2T_PROF_ATTN_FUSED_16) | \
                                (1ull << M2T_PROF_CONV3_BWD))
bool m2t_prof_take(hipEvent_t* a, hipEvent_t* b);
// an armed fork event (m2t_backward, option "fork_on_kernel") rides on the dispatch as its stop event instead of being recorded by
// a marker packet behind it; nullptr when none is armed or a timing pair already took the dispatch
hipEvent_t m2t_fork_take();
extern thread_local hipEvent_t g_m2t_fork_armed;      // (m2t_prof.hip; set and cleared by m2t_backward only)
#define M2T_LAUNCH_TIMED(kernel, grid, block, sh, st, ...)                                                       \
  do {                                                                                                           \
    hipEvent_t ea__, eb__;                                                                                       \
    if (m2t_prof_take(&ea__, &eb__)) hipExtLaunchKernelGGL(kernel, grid, block, sh, st, ea__, eb__, 0, __VA_ARGS__); \
    else if (hipEvent_t ef__ = m2t_fork_take()) hipExtLaunchKernelGGL(kernel, grid, block, sh, st, nullptr, ef__, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel, grid, block, sh, st, __VA_ARGS__);                                           \
  } while (0)
struct M2TProfScope {
  int cat; hipStream_t st;
  M2TProfScope(int c, hipStream_t s) : cat(c), st(s) { m2t_prof_begin(cat, st); }
  ~M2TProfScope() { m2t_prof_end(cat, st); }
};

// ---- k_local_norm.hip: local-window InstanceNorm statistics + apply (option "local_norm"): X (P64) -> Xn (P64), hs = B*H*W*64 fp64 pairs
int launch_local_norm(int dt, const void* X, void* hs, void* Xn, int B, int H, int W, int T, hipStream_t st);

// ---- k_health.hip: the step health record (option "health"): per (row, chunk) partials, then one fold per row and the header row
struct m2t_health_desc {   // one row: a workspace tensor, or (off < 0) the buffer the pass got from its caller (sr, grads)
  long long off, n;        // byte offset in the workspace, element count
  int dtype, phase;        // m2t_dtype of the stored elements; 0 = written by the forward, 1 = left by the backward
  int item0, nitems;       // the row's chunks in the work list (and in "health_part")
};
int launch_health_record(const void* ws, const void* ext, const m2t_health_desc* descs, const int* work, double* parts, double* rec,
                         int phase, int row0, int nrows, int item0, int nitems, hipStream_t st);

// ---- k_pointwise.hip --------------------------------------------------------------------
int launch_dwt(int dt, int L, const void* src, int lds_, int c0, void* dst, int ldd, int d0, int B, int H, int W,
               int C, bool inverse, hipStream_t st);
int launch_pixel_shuffle_nchw(const float* in, float* out, int B, int C, int H, int W, int r, int inverse, hipStream_t st);
int launch_instnorm_finalize(const float* part, float* mean, float* rstd, int B, int nsplit, hipStream_t st);
int launch_instnorm_stats(int dt, const void* x, float* mean, float* rstd, float* part, int B, int P, hipStream_t st);
int launch_branch_prep(int dt, int L, const void* x, const float* mean, const float* rstd, const void* xc, int k,
                       void* xin, void* d, int B, int H, int W, hipStream_t st);
int launch_branch_post(int dt, int L, const void* a, const void* xin, void* xc, int k, int B, int H, int W, hipStream_t st);
int launch_branch_post_bwd(int dt, int L, const void* gxc, int k, void* ga, int B, int H, int W, hipStream_t st);
// gdwin != nullptr: ring rows [window][36][16 * 4^L] of the fused projection data gradient, added to the border pixels on load
int launch_branch_prep_bwd(int dt, int L, const void* gd, void* gxc, void* gn, int k, int B, int H, int W, hipStream_t st,
                           const void* gdwin = nullptr);
// part0 != nullptr (bf16): the first reduction stage already ran inside launch_c16_dgrad_prep (its norm arguments): skip it
int launch_instnorm_bwd(int dt, const void* gn, const void* x, const float* mean, const float* rstd, const void* gres,
                        void* gx, float* part, float* s, int B, int P, hipStream_t st, const float* part0 = nullptr, int tiles0 = 0,
                        const void* gres2 = nullptr);       // gres2: a second residual gradient added in the same pass (block 0: g(Y) of `res + x`)
int launch_add(int dt, const void* a, const void* b, void* o, long long n, hipStream_t st);
int launch_colsum(int dt, const void* a, int lda, long long M, int N, float* part, int max_part_blocks, float* out,
                  int accumulate, hipStream_t st, int unshuf = 0, int gH = 0, int gW = 0, int gr = 1, int gC = 64,
                  int* nblk_out = nullptr);   // nblk_out != null: write the partials only and report their count
int launch_multi_reduce(const float* arena, float* grads, const m2t_red_desc* descs, int ndesc, hipStream_t st);
// loss_kind (M2TPixelLossKind) and its factors lparam / lf0 / lf1: m2t_pixel_loss.h (gscale carries mse's 2); the default is the L1 loss
int launch_clamp_l1(const float* pre, const float* hr, float* sr, float* gpre, float* part, float* loss, int B, int Hp,
                    int Wp, int Hs, int Ws, float R, float loss_scale, float gscale, hipStream_t st, int loss_kind = M2T_PL_L1,
                    float lparam = 0.f, float lf0 = 0.f, float lf1 = 0.f);
// loss = loss_scale * sum(part[0 .. n)) in a fixed order (n <= M2T_LOSS_BLOCKS)
int launch_loss_finish(const float* part, int n, float loss_scale, float* loss, hipStream_t st);
int launch_adam(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps,
                int step, float gscale, hipStream_t st);
// acc[0 .. n) += g (one fp32 addition per element); loss_acc[0] += loss_part[0] when both are given (same launch)
int launch_grad_accumulate(float* acc, const float* g, long long n, float* loss_acc, const float* loss_part, hipStream_t st);
// ---- k_optim.hip: gradient norm -> optimizer record; Adam with clip / weight decay / EMA / skip in one pass
#define M2T_GNORM_BLOCKS 256          // workgroups (= fp64 partials) of the norm's first stage: a constant, so the tree depends on n alone
#define M2T_GNORM_THREADS 1024       // threads per workgroup of that stage (a constant for the same reason)
#define M2T_OPTIM_RECORD_DOUBLES 8    // norm, finite, clip_coef, applied, skipped, bc1, sqrt(bc2), effective step
int launch_grad_norm(const float* g, long long n, float gscale, float max_norm, int skip_nonfinite, int step, float b1, float b2,
                     double* rec, double* part, hipStream_t st);
// ema / rec may be nullptr (no EMA; no clip, no skip, host bias correction from `step`)
int launch_adam_ex(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float b1, float b2, float eps,
                   int step, float gscale, float wd, int decoupled, float ema_d, const double* rec, hipStream_t st);
// blocks: device table int2[nblocks] = (descriptor index, chunk of M2T_PACK_CHUNK output elements)
int launch_pack(int dt, const float* master, void* packed, const m2t_pack_desc* descs, const void* blocks, int nblocks, hipStream_t st);
int launch_layout(int dt, const float* nchw, void* nhwc, float* nchw_out, int B, int C, int HW, int inverse, hipStream_t st);

// ---- k_gemm.hip -------------------------------------------------------------------------
// Y[M][N] = A[M][K] * W[N][K]^T  with A-side and epilogue variants
// leading dimension sentinel: the operand / output is a P64 feature map ([4][M][16], m2t_common.h) with M rows
#define M2T_LD_P64 (-64)
enum m2t_gemm_a { M2T_A_PLAIN = 0, M2T_A_GELU = 1, M2T_A_UNSHUF = 2 };
enum m2t_gemm_epi { M2T_E_PLAIN = 0, M2T_E_BIAS = 1, M2T_E_BIAS_SHUF = 2, M2T_E_GELU_GRAD = 3, M2T_E_BIAS_GELU = 4, M2T_E_BIAS_RESID = 5,
                    M2T_E_BIAS_RELU = 6 };   // (+ bias, ReLU: Mlp of util/rlutrans.py:22-23)
struct m2t_gemm_args {
  const void* A; int lda;       // A rows (or, UNSHUF: the [B][H*r][W*r][C] tensor)
  const void* W;                // [N][K] element type T
  void* Y; int ldy;             // output (or, SHUF: the [B][H*r][W*r][C] tensor)
  const float* bias;            // [N] fp32 (E_BIAS*)
  const void* aux; int ldaux;   // E_GELU_GRAD: stored derivative gelu'(t), same shape as Y; E_BIAS_RESID: residual
  void* Y2 = nullptr;           // E_BIAS_SHUF: second output, the derivative gelu'(t) (Y receives gelu(t))
  long long M; int N, K;
  int H, Wd, r, C;              // shuffle geometry: rows m = (b, h, w) over [B][H][Wd]; C channels after shuffle
  const void* halo_win = nullptr;   // M2T_A_HALO: per-window dK|dV scratch (H, Wd = branch grid, C = branch channels)
};
int launch_gemm_nt(int dt, int amode, int emode, const m2t_gemm_args& a, hipStream_t st);
// fp32 (parity mode): 1 = the v_mfma_f32_32x32x2_f32 kernels of round 5 for the plain GEMMs, the qkv weight gradients and the 3x3 conv,
// 0 = the 16x16x4 kernels of rounds 1-4 (option fp32_fast of the plan being run; set by m2t_api.hip on entry)
extern thread_local int g_m2t_f32_fast;
// upsampler 1x1 conv + bias + pixel-shuffle scatter + GELU, K = 64, N = 64 r^2; X rows over [B][H][Wd];
// Y = gelu(t), Yd = gelu'(t) (both [B][H r][Wd r][64]); Yd == nullptr: the derivative is not stored (inference plans)
int launch_tail_expand(int dt, const void* X, const void* Wp, const float* bias, void* Y, void* Yd, long long M, int H, int Wd,
                       int r, bool x_p64, hipStream_t st);   // x_p64: X is a P64 feature map (else rows of 64)
// dW[N][K] (fp32 slabs) = sum_m G[m][N]^T X[m][K];  G/X side variants as above
struct m2t_wgrad_args {
  const void* G; int ldg; int gmode;   // M2T_A_PLAIN or M2T_A_UNSHUF
  const void* X; int ldx; int xmode;   // M2T_A_PLAIN or M2T_A_GELU
  float* slabs;                        // [nslab][N][K]
  float* bias_slabs;                   // optional [nslab][N]: column sums of G (bias gradient)
  long long M; int N, K;
  int H, Wd, r, C;
  const void* halo_win = nullptr;
  int big_tiles = 0;                   // > 0: bf16 plain / plain, N % 128 == 0, K % 128 == 0: 128 x 128 output tiles (wgrad_tn_big_kernel),
                                       // value = target number of workgroups (tiles x slabs), 64 .. 512
};
int launch_wgrad_tn(int dt, const m2t_wgrad_args& a, int* nslab_out, hipStream_t st);
int wgrad_slab_count(long long M, int N, int K);   // upper bound of the slabs launch_wgrad_tn will write

// ---- k_conv.hip -------------------------------------------------------------------------
int launch_head_conv_fwd(int dt, const float* x, const float* w, const float* b, void* out, int B, int H0, int W0,
                         int H, int W, hipStream_t st);
int launch_head_im2col(int dt, const float* x, void* cols, int B, int H0, int W0, int H, int W, hipStream_t st);   // cols [B*H*W][32] (T)
// d x of the head conv (through both reflect pads): g P64 (T) [4][B*H*W][16] -> gx fp32 NCHW [B][3][H0][W0]; deterministic gather
int launch_head_conv_dgrad(int dt, const void* g, const float* w, float* gx, int B, int H0, int W0, int H, int W, hipStream_t st);
// 64->64 3x3, zero padding.  wp: packed [9][64 out][64 in] (T). y = conv(x) + bias + res1 + res2 (each optional)
int launch_conv3x3_c64(int dt, const void* x, const void* wp, const float* bias, const void* res1, const void* res2,
                       void* y, int B, int H, int W, hipStream_t st,
                       const void* wrows = nullptr,       // bf16: the same weight in M2T_PACK_CONV3_ROWS(_T) order and ...
                       const void* zero_page = nullptr,   // ... >= 64 zero bytes in device memory -> the row-streaming kernel
                       int variant = 0,                   // 0: row-streaming, DMA depth 2 (default); 1: the tile kernel
                                                          // (conv3x3_c64_pipe_kernel); 3: depth 3; 4: depth 2 + pipelined epilogue
                       float* stat_part = nullptr);       // one residual, row-streaming: InstanceNorm partials of y, [B][n][64][3] with
                                                          // n = conv3x3_c64_stat_partials(...) (0: this shape / variant cannot)
int conv3x3_c64_stat_partials(int dt, int B, int H, int W, int variant);
int launch_conv3x3_c64_wgrad(int dt, const void* x, const void* gy, float* slabs, float* bias_slabs, int* nslab, int B, int H,
                             int W, hipStream_t st);   // bias_slabs [nslab][64]: column sums of gy
// bf16: data gradient + weight / bias gradient partials in one pass over gy (conv3x3_c64_bwd_rows_kernel); M2T_UNSUPPORTED for
// shapes without a strip decomposition.  wrows_t: M2T_PACK_CONV3_ROWS_T; slabs [<= 256][9][64][64], bias_slabs [<= 256][64]
bool conv3x3_c64_bwd_fusable(int B, int H, int W);
int launch_conv3x3_c64_bwd_fused(const void* gy, const void* x, const void* wrows_t, void* gx, float* slabs, float* bias_slabs, int* nslab,
                                 const void* zero_page, int B, int H, int W, hipStream_t st);
// tail conv 64->3, reflect padding, input = the stored activation gelu(t); output NCHW fp32 [B][3][H][W]
int launch_final_conv_fwd(int dt, const void* tpre, const float* w, float* out, int B, int H, int W, hipStream_t st);
int launch_final_conv_dgrad(int dt, const float* gout, const float* w, const void* tpre, void* gtpre, int B, int H, int W,
                            hipStream_t st);
int launch_final_conv_wgrad(int dt, const float* gout, const void* tpre, float* slabs, int* nslab, int B, int H, int W,
                            hipStream_t st);

// ---- k_branch.hip -----------------------------------------------------------------------

// ---- k_tail_fwd.hip ----------------------------------------------------------------------
// x4 tail, bf16: tail.3 expansion + PixelShuffle + GELU + tail conv in one pass; gelu(t2) never reaches HBM.
int launch_tail_fwd_fused(const void* a1, const void* w3p, const float* b3, const float* wf, float* out, int B, int H, int W,
                          hipStream_t st);

// ---- k_tail_stream.hip -------------------------------------------------------------------
// bf16: expansion 1x1 (64 -> 64 R^2) + PixelShuffle(R) + GELU + tail conv as ONE row-streaming kernel; R = 2 (x4's tail.3 stage on the
// NHWC mid-resolution map, or x2's tail.0 stage on the P64 body output) or 3 (x3).  seg_rows <= 2: default segment length.
int launch_tail_fwd_stream(const void* a, int a_is_p64, const void* wp, const float* bias, const float* wf, float* out, int B, int Hi,
                           int Wi, int R, int seg_rows, hipStream_t st);

// ---- k_tail_bwd_stream.hip ---------------------------------------------------------------
// bf16: the recomputing backward of the tail's last stage as a row-streaming kernel (round 4).  tail0 = 1 (R = 2 / 3): x2's / x3's whole
// tail on the P64 body output; tail0 = 0 (R = 2): x4's tail.3 stage (kept for A/B: slower than the tile kernel).  Hi, Wi: size of the
// expansion's INPUT map.  Slabs: tail_bwd_stream_blocks() of each kind.
int tail_bwd_stream_blocks(int B, int Hi, int Wi, int R);
int launch_tail_bwd_stream(const float* gout, const float* wf, const void* a, const void* d1, const void* w3t, const float* b3, void* ga,
                           float* slab_wf, float* slab_w3, float* slab_b3, int* nslab_out, int B, int Hi, int Wi, int R, int tail0,
                           hipStream_t st);

// ---- k_tail_bwd.hip ----------------------------------------------------------------------
// x4 tail, bf16: tail conv data + weight gradient, GELU backward, tail.3 data + weight + bias gradient in one pass
// over the stored activation / derivative tensors (g(t2) never reaches HBM).  Slabs: wf [n][32][64], w3 [n][256][64],
// b3 [n][256]; n = *nslab_out <= tail_bwd_fused_blocks().
int tail_bwd_fused_blocks(int B, int H, int W);
// act == der == nullptr: gelu(t2) / gelu'(t2) are recomputed per tile from a1, w3t and the tail.3 bias b3 (torch order)
// l1_pre != nullptr (recomputing variant only): the clamp + L1 seed of launch_clamp_l1 is taken inside the kernel from the pre-clamp
// output l1_pre [B][3][H][W] and the target l1_hr [B][3][Hs][Ws] (gout is then unused); l1_part [tail_bwd_fused_blocks] receives the
// partial sums of |clamp(pre) - hr| for launch_loss_finish.  loss_kind / lparam / lf0 / lf1 as launch_clamp_l1's: the same per-pixel function
// (m2t_pixel_loss.h), so the seed taken inside and the stand-alone one cannot drift apart
int launch_tail_bwd_fused(const float* gout, const float* wf, const void* act, const void* der, const void* a1, const void* d1,
                          const void* w3t, const float* b3, void* gt1, float* slab_wf, float* slab_w3, float* slab_b3,
                          int* nslab_out, int B, int H, int W, hipStream_t st, const float* l1_pre = nullptr, const float* l1_hr = nullptr,
                          float* l1_part = nullptr, int Hs = 0, int Ws = 0, float R = 0.f, float gscale = 0.f, int variant = 32,
                          int loss_kind = M2T_PL_L1, float lparam = 0.f, float lf0 = 0.f, float lf1 = 0.f);
// variant (recomputing form): 32 = the round-6 kernel on v_mfma_f32_32x32x16_bf16 (conflict-free LDS operand reads, g(t2) formed in
// registers; results agree with the older kernel to fp32 summation order), 16 = the 16x16x32 kernel of rounds 2-5 (what the stored
// form always runs)

// ---- k_attn.hip -------------------------------------------------------------------------
// qkv [B][h][w][3C] (q | k | v), rel_h/rel_w fp32 [10][C/2];  out rows at ldo (+ optional residual rows at ldr)
// post_levels = 1, 2: out/res are the FULL-RES xc (ld ldo, channel offset oc0) / xin (ld ldr) tensors and the
// epilogue writes xc = IWT^levels(attention) + xin
int launch_window_attn_fwd(int dt, const void* qkv, const float* rel_h, const float* rel_w, void* out, int ldo, int oc0,
                           const void* res, int ldr, int B, int h, int w, int C, hipStream_t st, int post_levels = 0);
// gout [B][h][w][ldg] (channels gc0..gc0+C) -> gqkv [B][h][w][3C]; `win` [windows][36][2C] (T): the dK|dV rows of each
// window's 36 ring keys (its own 64 pixels are written straight to gqkv; halo_gather adds the ring rows to the
// border pixels of the neighbouring windows);
// rel-pos gradient slabs
int launch_window_attn_bwd(int dt, const void* qkv, const float* rel_h, const float* rel_w, const void* gout, int ldg,
                           int gc0, void* gqkv, void* win, float* relw, int B, int h, int w, int C, hipStream_t st,
                           int dwt_levels = 0,    // 1, 2: gout is the FULL-RES g_xc tensor; DWT^levels applied on load
                           bool gather = true,    // false: skip the halo gather (border pixels then lack their neighbours' ring rows)
                           bool resident = true); // bf16, C = 64 / 256: whole-window-resident kernel (k_attn_res.hip)
// C = 16, bf16, no fused DWT: one wave per window (k_attn_c16.hip)
int launch_window_attn_fwd_c16(const void* qkv, const float* rel_h, const float* rel_w, void* out, int ldo, int oc0, const void* res,
                               int ldr, int B, int h, int w, hipStream_t st);
// d != nullptr (with wqkv = the packed [48][16] weight, M2T_PACK_COPY): qkv was not saved (may be nullptr); q | k | v are
// recomputed from the branch input d [pixel][16] with the forward kernel's own products (identical bits)
int launch_window_attn_bwd_c16(const void* qkv, const float* rel_h, const float* rel_w, const void* gout, int ldg, int gc0,
                               void* gqkv, void* win, float* relw, int B, int h, int w, hipStream_t st, const void* d = nullptr,
                               const void* wqkv = nullptr);
// k_attn_fwd2.hip (round 5): the same fused C = 256 forward branch as launch_window_attn_fused_prep_fwd, built for two workgroups per
// CU (4 waves, 80 KB of LDS, channel-chunked projection, scores in registers); vring [B (h/8)(w/8)][36][256]: scratch for the ring
// keys' v rows (window_attn_fwd2_vring_elems elements)
size_t window_attn_fwd2_vring_elems(int B, int h, int w);
int launch_window_attn_fused_prep_fwd2(const void* xn, const void* xprev, const float* mean, const float* rstd, int k, void* xin, void* d,
                                       const void* wfrag, const float* rel_h, const float* rel_w, void* qkv, void* out, void* vring,
                                       int B, int h, int w, int windows_per_wg, hipStream_t st, int stagger = 0);
// bf16 C = 16 branch: halo gather + projection data gradient + branch_prep_bwd (k = 0) in one kernel (k_attn_c16.hip)
// nx != nullptr (round 5): the first stage of the InstanceNorm backward rides in the same launch -- extra workgroups sum planes 1 .. 3
// of g_n (complete by then) into npart [B][M2T_NORM_SPLIT][64][2], and every tile leaves the plane-0 sums of its 16 pixels in
// npart0 [tile][2][16]; gn / nx are then the FULL P64 tensors (plane 0 first), mean / rstd [B][64]
int launch_c16_dgrad_prep(void* gqkv, const void* win, const void* wT, const void* gxc, void* gn, int B, int h, int w, hipStream_t st,
                          const void* nx = nullptr, const float* mean = nullptr, const float* rstd = nullptr, float* npart = nullptr,
                          float* npart0 = nullptr);
int launch_window_attn_fwd_resident(const void* qkv, const float* rel_h, const float* rel_w, void* out, int ldo, int oc0,
                                    const void* res, int ldr, int B, int h, int w, int C, int post_levels, hipStream_t st);
// the resident kernel alone (bf16); M2T_UNSUPPORTED when (C, dwt_levels) has no instantiation
// wdfrag != nullptr ((C, dwt_levels) = (256, 2) or (64, 1)): the data gradient of the qkv projection is taken in the same
// launch -- wdfrag = Wqkv^T as MFMA fragments (M2T_PACK_FRAG16_T); own pixels' rows -> gd [pixel][C], the 36 ring keys'
// rows -> gdwin [window][36][C] (added to the border pixels by launch_halo_gather(gdwin, gd, .., C, C, 0))
int launch_window_attn_bwd_resident(const void* qkv, const float* rel_h, const float* rel_w, const void* gout, int ldg, int gc0,
                                    void* gqkv, void* win, float* relw, int B, int h, int w, int C, int dwt_levels, hipStream_t st,
                                    const void* wdfrag, void* gd, void* gdwin,
                                    // (C, dwt_levels) = (64, 1) with the fused data gradient: xsrc [pixel][C] = the branch input and wfrag = Wqkv as
                                    // M2T_PACK_FRAG16: qkv was not saved (may be nullptr), q | k | v are recomputed (identical bits)
                                    const void* xsrc = nullptr, const void* wfrag = nullptr,
                                    // (256, 2) with pb_gd != nullptr: branch_prep_bwd of the NEXT branch k = i + 1 inside (its own-window g_d rows, their
                                    // ring rows, plane k of g_xc, plane k of g_n (written)); gout = plane i of g_xc is then updated in place
                                    const void* pb_gd = nullptr, const void* pb_gdwin = nullptr, const void* pb_gxk = nullptr, void* pb_gnk = nullptr);
int launch_halo_gather(int dt, const void* win, void* dst, int B, int h, int w, int rw, int ld, int coff, hipStream_t st);
// k_attn_c16.hip: the whole C = 16 branch forward (InstanceNorm apply of chunk 0 + qkv projection + attention + residual), bf16.
// x = chunk-0 plane of the block input; wqkv [48][16] (M2T_PACK_COPY); d [B*h*w][16] and qkv [B*h*w][48] are WRITTEN
// (qkv == nullptr: not saved -- launch_window_attn_bwd_c16 then recomputes it from d)
int launch_window_attn_fused_c16_fwd(const void* x, const float* mean, const float* rstd, const void* wqkv, const float* rel_h,
                                     const float* rel_w, void* d, void* qkv, void* out, int ldo, int oc0, int B, int h, int w,
                                     hipStream_t st);
// k_attn_fused.hip: qkv projection + window attention + IWT / residual epilogue in one kernel (bf16, C = 64 / 256).
// x [B][h][w][C]; wfrag = the [3C][C] qkv weight in M2T_PACK_FRAG16 order; qkv [B][h][w][3C] is WRITTEN (saved for the backward)
int launch_window_attn_fused_fwd(const void* x, const void* wfrag, const float* rel_h, const float* rel_w, void* qkv, void* out,
                                 int ldo, int oc0, const void* res, int ldr, int B, int h, int w, int C, int post_levels,
                                 hipStream_t st);
int launch_window_attn_fused_prep_fwd(const void* xn, const void* xprev, const float* mean, const float* rstd, int k, void* xin, void* d,
                                      const void* wfrag, const float* rel_h, const float* rel_w, void* qkv, void* out, int B, int h, int w,
                                      int C, int post_levels, hipStream_t st);
// relw [nwin][10][C] per-window partials -> grel_h / grel_w (torch layouts)
int launch_rel_reduce(const float* relw, float* rel_part, float* grel_h, float* grel_w, int nwin, int C, hipStream_t st);
int launch_rel_reduce1(const float* relw, float* rel_part, int nwin, int C, int* nsplit_out, hipStream_t st);

// ---- k_swin.hip (MedCLIP image tower = Swin-T forward, losses.py:68-69) --------------------
int launch_swin_patchify(int dt, const float* src, const float* src_b, int n_a, int Hs, int Ws, const int* crops, int n, void* out,
                         hipStream_t st);
int launch_layernorm(int dt, const void* x, const float* gamma, const float* beta, void* y, long long M, int C, hipStream_t st,
                     float eps = 1e-5f);     // (Swin / TransBlock: 1e-5; BERT: 1e-12)
// fused Swin MLP (bf16, C = 96 / 192): X <- X + fc2(gelu(fc1(LayerNorm(X)) + b1)) + b2, weights in FRAG16 order
int launch_swin_mlp_fused(void* X, const float* gamma, const float* beta, const void* w1f, const float* b1, const void* w2f,
                          const float* b2, long long M, int C, hipStream_t st);
int launch_frag16_pack(int dt, const float* src, void* dst, int N, int K, hipStream_t st);
int launch_swin_attn(int dt, const void* qkv, const float* bias_table, void* out, int nimg, int H, int W, int C, int heads,
                     int shift, hipStream_t st);
int launch_swin_merge_gather(int dt, const void* x, void* y, int nimg, int H, int W, int C, hipStream_t st);
int launch_swin_head(int dt, const void* x, const float* proj, float* emb, int nimg, hipStream_t st);
int launch_semantic_loss(const float* emb, const float* text, int B, int n_patches, float* per_sample, float* total, hipStream_t st);
int launch_bicubic_resize(const float* src, float* dst, int NC, int Hin, int Win, int Hout, int Wout, hipStream_t st);
int launch_convert(int dt, const float* src, void* dst, long long n, hipStream_t st);
// ---- k_swin_bwd.hip (data gradient of the image tower: the opt-in differentiable SemanticLoss) ----------
struct M2TCropOrigins { int y0[64], x0[64]; };   // per-sample block origins of one add_output_grad launch (<= 64 samples)
int launch_semantic_loss_bwd(const float* emb, const float* text, int B, int n_patches, float* g_emb, hipStream_t st);
int launch_swin_head_bwd(int dt, const void* hn, const float* proj, const float* g_emb, void* g_hn, int nimg, hipStream_t st);
int launch_layernorm_bwd(int dt, const void* x, const void* g, const float* gamma, const float* resid, float* out_f, void* out_t,
                         long long M, int C, hipStream_t st, float eps = 1e-5f, const float* g_f = nullptr);
int launch_swin_attn_bwd(int dt, const void* qkv, const float* bias_table, const void* gout, void* gqkv, int nimg, int H, int W, int C,
                         int heads, int shift, hipStream_t st);
int launch_swin_merge_scatter(int dt, const float* gy, float* gx, void* gxt, int nimg, int H, int W, int C, hipStream_t st);
int launch_swin_embed_bwd(const float* ge, const float* wpe, float* g_crops, int nimg, hipStream_t st);
int launch_transpose_convert(int dt, const float* src, void* dst, int N, int K, int ldd, int col0, hipStream_t st);
int launch_bicubic_resize_bwd(const float* gdst, float* gsrc, int NC, int Hin, int Win, int Hout, int Wout, hipStream_t st);
int launch_add_output_grad(const float* pre, const float* g, float* gpre, int B, int Hp, int Wp, int gh, int gw, const M2TCropOrigins& org,
                           float scale, float R, hipStream_t st);
// ---- k_rlutrans_bwd.hip (the TransBlock backward: include/m2t_rlutrans.h, host layer m2t_rlutrans.hip) ----------
// gh1 [M][16] = [h1 > 0] * (gy [M][64] . w2 [64][16]), all in the storage type
int launch_tb_fc2_dgrad_relu(int dt, const void* gy, const void* w2, const void* h1, void* gh1, long long M, hipStream_t st);
// backward of the chunked attention (chunks of N / 16 tokens): qkv [M][192], ao / gao [M][64] -> gqkv [M][192]; stats: M * 8 * 3 floats of scratch
int launch_tb_attn_bwd(int dt, const void* qkv, const void* ao, const void* gao, void* gqkv, float* stats, long long M, int N, hipStream_t st);
// LayerNorm (C = 64, eps 1e-5) affine gradients, first stage: part [*nblk_out][128] = (sum g xhat | sum g) per block of rows
int launch_tb_ln_affine(int dt, const void* x, const void* g, float* part, long long M, int* nblk_out, hipStream_t st);
// second stage of all parameter gradients in one launch; the descriptors ride in the kernel arguments (no device table to upload)
struct tb_reduce_desc { long long src, dst; int n, ns; };     // out[dst + e] = sum_{s < ns} arena[src + s n + e], e < n
struct tb_reduce_table { tb_reduce_desc d[12]; };
int launch_tb_param_reduce(const float* arena, float* out, const tb_reduce_table& tab, int ndesc, hipStream_t st);
// ---- k_ssim_loss.hip (the 1 - SSIM loss term and its gradient: m2t_ssim_loss_tensor / m2t_ssim_loss) ----------
// x [B][C][H][W] with image stride xs_img, channel stride xs_img / C, row stride xs_row; y contiguous; gx_add (or nullptr) has x's strides:
// gx_add[q] += -scale * d sum(S) / dx[q] (through the clamp mask when clamp); loss_out = (accumulate ? loss_out : 0) + scale * sum(1 - S).
// scratch: ssim_loss_scratch_bytes(B, C, H, W) bytes (0 when H or W < 11).  Arguments are checked by the callers.
size_t ssim_loss_scratch_bytes(int B, int C, int H, int W);
// The refusals the plan-free m2t_<term>_loss_tensor entries share, in the order they always made them: null argument, the term's batch /
// size rule, data_range, the term's further argument rule, the strides of x.  The two rules of the term are decided at the call site and
// come in as the refusal's text (nullptr: passed); `who` prefixes every message.  0 or M2T_ERR_ARG.
int loss_tensor_check(const char* who, const float* x, const float* y, const float* loss_out, const void* scratch, int C, int H, int W,
                      long long x_image_stride, int x_row_stride, float data_range, const char* shape_refusal,
                      const char* more_refusal = nullptr);
// The last launch of every loss term, one workgroup, fixed order: loss_out = (accumulate ? loss_out : 0) + (float)(scale * sum_i v_i),
// v_i = p[i * stride] for i < n, or 1 - p[i * stride] with one_minus.
int launch_loss_finish(const double* p, long long n, long long stride, int one_minus, double scale, int accumulate, float* loss_out,
                       hipStream_t st);
template <typename K>
int ensure_lds(K kernel, size_t bytes) { return m2t_ensure_dynamic_lds((const void*)kernel, (int)bytes); }
// The scratch of a levelled term (MS-SSIM, VIF), offsets in doubles: the records | the tiles' partial sums per level | the planes
// a, b (both pyramids) and g (the gradient) of levels 1 .. (index 0 of a / b / g is unused).  The term sets levels and h / w / ty / tx
// by its own size rule; levelled_layout_fill(items, rec, sums) places `rec` doubles per item, `sums` per tile and item, and the planes.
struct LevelledLayout {
  static constexpr int MAX_LEVELS = 5;
  int levels, h[MAX_LEVELS], w[MAX_LEVELS], ty[MAX_LEVELS], tx[MAX_LEVELS];
  size_t rec, part[MAX_LEVELS], a[MAX_LEVELS], b[MAX_LEVELS], g[MAX_LEVELS], total;
};
void levelled_layout_fill(LevelledLayout& L, size_t items, int rec, int sums);
// bytes into the scratch of region 0 (records), 1 (partial sums of `level`), 2 / 3 / 4 (planes a / b / g of `level` >= 1); (size_t)-1: none
size_t levelled_layout_offset(const LevelledLayout& L, int region, int level);
void ssim_loss_taps(double* g11);      // the 11 taps of the window (the fp32 taps torch builds, widened), also those of k_msssim_loss.hip
int launch_ssim_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                     double scale, float* gx_add, float* loss_out, int accumulate, void* scratch, hipStream_t st);
// ---- k_msssim_loss.hip (the 1 - MS-SSIM loss term and its gradient: m2t_msssim_loss_tensor / m2t_msssim_loss) ----------
// The strides, gx_add, loss_out and accumulate of launch_ssim_loss; loss_out = (accumulate ? loss_out : 0) + scale * sum_bc (1 - M_bc);
// per_channel_out (or nullptr): double [B*C] = M_bc.  scratch: msssim_loss_scratch_bytes(B, C, H, W) bytes (0 when min(H, W) <= 160 or
// B * C is outside 1 .. 65535).  Arguments are checked by the callers.
bool msssim_loss_size_supported(int H, int W);
size_t msssim_loss_scratch_bytes(int B, int C, int H, int W);
int launch_msssim_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                       double scale, float* gx_add, float* loss_out, double* per_channel_out, int accumulate, void* scratch,
                       hipStream_t st);
// ---- k_vif_loss.hip (the 1 - VIF loss term and its gradient: m2t_vif_loss_tensor / m2t_vif_loss) ----------
// The strides, gx_add, loss_out and accumulate of launch_ssim_loss; C is 1 or 3 (one luminance plane per image);
// loss_out = (accumulate ? loss_out : 0) + scale * sum_b (1 - VIF_b); per_image_out (or nullptr): double [B] = VIF_b.
// scratch: vif_loss_scratch_bytes(B, C, H, W) bytes (0 when min(H, W) < 41, C is not 1 or 3, or B is outside 1 .. 65535).
bool vif_loss_size_supported(int H, int W);
size_t vif_loss_scratch_bytes(int B, int C, int H, int W);
int launch_vif_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, double sigma_n_sq,
                    int clamp, double scale, float* gx_add, float* loss_out, double* per_image_out, int accumulate, void* scratch,
                    hipStream_t st);
// ---- k_gmsd_loss.hip (the GMSD loss term and its gradient: m2t_gmsd_loss_tensor / m2t_gmsd_loss) ----------
// The strides, gx_add, loss_out and accumulate of launch_ssim_loss; C is 1 or 3 (one pooled luminance plane per image);
// loss_out = (accumulate ? loss_out : 0) + scale * sum_b GMSD_b; per_image_out (or nullptr): double [B] = GMSD_b.
// scratch: gmsd_loss_scratch_bytes(B, C, H, W) bytes (0 when H or W < 2, C is not 1 or 3, or B is outside 1 .. 65535).
bool gmsd_loss_size_supported(int H, int W);
size_t gmsd_loss_scratch_bytes(int B, int C, int H, int W);
int launch_gmsd_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                     double scale, float* gx_add, float* loss_out, double* per_image_out, int accumulate, void* scratch, hipStream_t st);
// ---- k_wavelet_loss.hip (the wavelet-domain loss term, its gradient and the transform alone: m2t_swt2 / m2t_wavelet_loss_tensor /
// m2t_wavelet_loss) ----------
// The strides, gx_add, loss_out and accumulate of launch_ssim_loss; lo / hi [taps] and band_weights [3 levels + 1] (or nullptr: 1 for
// every detail band, 0 for LL) are HOST arrays read at call time; per_band_out (or nullptr): double [3 levels + 1], the unweighted
// band sums (0 for a band of weight 0).  swt_out != nullptr: only the transform of x, fp32 [B][C][3 levels + 1][H][W] (y may be null).
// The refusals return the text of the first rule broken, nullptr when none is.
const char* wavelet_shape_refusal(int B, int C, int H, int W, int levels, int taps);
const char* wavelet_filter_refusal(const double* lo, const double* hi, int taps, int levels, const double* band_weights, double eps);
size_t wavelet_loss_scratch_bytes(int B, int C, int H, int W, int levels, int taps);
int launch_wavelet_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp,
                        double scale, const double* lo, const double* hi, int taps, int levels, const double* band_weights, double eps,
                        float* swt_out, float* gx_add, float* loss_out, double* per_band_out, int accumulate, void* scratch,
                        hipStream_t st);
// ---- k_consistency.hip (LR-consistency: m2t_consistency_loss_tensor / m2t_consistency_loss / m2t_back_project_f32) ----------
// x [B][C][H s][W s] with the strides of launch_ssim_loss, y contiguous [B][C][H][W] (the LR side); gx_add, loss_out and accumulate of
// launch_ssim_loss; stats_out (or nullptr): double [3] = {mean |r|, max |r|, mean r^2}.  scratch: consistency_scratch_bytes(B, C, H, W, s)
// bytes (0 for an unsupported shape).  Arguments are checked by the callers.
size_t consistency_scratch_bytes(int B, int C, int H, int W, int s);
int launch_consistency_loss(const float* x, const float* y, int B, int C, int H, int W, int s, long long xs_img, int xs_row, float R,
                            int clamp, double eps, double scale, float* gx_add, float* loss_out, double* stats_out, int accumulate,
                            void* scratch, hipStream_t st);
// ---- k_fft_loss.hip (the L1 loss on the coefficients of a 2-D real FFT and its gradient: m2t_fft_loss_tensor / m2t_fft_loss) ----------
// x [B][C][H][W] with image stride xs_img, channel stride xs_img / C, row stride xs_row; y contiguous; gx_add (or nullptr) has x's strides:
// gx_add[q] += scale * d sum(|Re D| + |Im D|) / dx[q] (through the clamp mask when clamp); loss_out = (accumulate ? loss_out : 0) + scale * sum.
// norm 0 = "backward", 1 = "ortho".  scratch: fft_loss_scratch_bytes(B, C, H, W) bytes (0 for an unsupported size).  Arguments are
// checked by the callers.
bool fft_loss_size_supported(int H, int W);
size_t fft_loss_scratch_bytes(int B, int C, int H, int W);
int launch_fft_loss(const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R, int clamp, int norm,
                    double scale, float* gx_add, float* loss_out, int accumulate, void* scratch, hipStream_t st);
// ---- k_vgg.hip (the VGG19 feature loss: include/m2t_perceptual.h, host layer m2t_vgg.hip) ----------
// bf16 NHWC activations, packed bf16 weights [Cout / 64][Cin / 32][9][64][32]; Cin and Cout multiples of 64.  epi 0: bias + ReLU;
// epi 1 (data gradient on flipped, transposed weights): + sd.gscale * rho'(mask - ytap) where ytap != nullptr, times [mask > 0] where
// mask != nullptr.  Arguments are checked by the callers.
int launch_vgg_conv(int epi, const void* in, const void* wpk, void* out, int N, int H, int W, int Cin, int Cout, const float* bias,
                    const void* mask, const void* ytap, const M2TPixelLoss& sd, hipStream_t st);
int launch_vgg_pack(const float* w, void* dst, int Cout, int Cin, int flip, hipStream_t st);
int launch_vgg_pack_first(const float* w, float* dst, hipStream_t st);
// conv1_1 on (c(x) / R - mean) / std (chs = channel stride, 0 repeats one channel) and its data gradient, added into gx
int launch_vgg_first_fwd(const float* x, long long img, long long chs, int row, float R, int clamp, const float* w0, const float* bias,
                         void* out, int N, int H, int W, hipStream_t st);
int launch_vgg_first_bwd(const void* g, const float* w0, const float* x, float* gx, long long img, long long chs, int row, float R, int clamp,
                         int N, int H, int W, hipStream_t st);
int launch_vgg_pool_fwd(const void* in, void* out, int N, int H, int W, int C, hipStream_t st);
int launch_vgg_pool_bwd(const void* a, const void* gout, void* gin, int N, int H, int W, int C, int relu, hipStream_t st);
int vgg_tap_blocks(long long n_elems);
int launch_vgg_tap_partial(const void* fx, const void* fy, long long n_elems, const M2TPixelLoss& sd, double* part, hipStream_t st);
int launch_vgg_finish(const double* part, const int* nblk, const double* wn, const double* inv_n, int accumulate, float* loss_out,
                      double* per_tap_out, hipStream_t st);
int launch_vgg_tap_seed(const void* fx, const void* fy, long long n_elems, const M2TPixelLoss& sd, void* gout, hipStream_t st);
// ---- m2t_vgg.hip: the routine behind m2t_vgg_loss_tensor and m2t_vgg_loss (tap k's mean divides by divisor * C_k H_k W_k) ----------
struct m2t_vgg;
bool vgg_loaded(const m2t_vgg* v);
bool vgg_size_supported(int H, int W);
int vgg_check_common(const char* who, const double* tw, double scale, float R, int kind, float param);
int launch_vgg_loss(const m2t_vgg* v, const float* x, const float* y, int B, int C, int H, int W, long long xs_img, int xs_row, float R,
                    int clamp, int kind, float param, const double* tw, double scale, double divisor, float* gx_add, float* loss_out,
                    double* per_tap_out, int accumulate, void* workspace, hipStream_t st);
