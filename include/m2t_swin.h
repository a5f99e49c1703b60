/* m2t_swin.h -- the MedCLIP image tower of m2t.h (m2t_swin_*), readable stage by stage: the encode call with its hidden states and
 * the backward call with its residual-stream gradients as extra outputs.  A seventeenth header on the same library, under the
 * conventions of m2t.h (extern "C", raw device pointers, a hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result,
 * m2t_last_error_string for the text); the sixteen older headers keep their entries.
 *
 * Together with the "ws:" / "wsn:" / "gws:" / "gwsn:" keys of m2t_swin_query this makes the input of every stage of both forward
 * paths and of the backward visible after one call: tests/test_gpu_swin_stages.py compares each kernel of the tower with fp64 on them. */
#ifndef M2T_SWIN_H
#define M2T_SWIN_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* m2t_swin_encode_pair with observation points (m2t_swin_encode and m2t_swin_encode_pair are this call with hidden_out = NULL;
 * the kernels and emb's bits are the same).  hidden_out (device, may be NULL) receives, for ALL n crops and in the compute
 * type, the tensors below one after the other, each [n][elements per crop], copied on the call's stream.  With T_s = 3136 / 4^s
 * token rows and C_s = 96 . 2^s channels at stage s (blocks per stage 2, 2, 6, 2):
 *   e0                       3136 x 96      patch projection, before the embedding LayerNorm
 *   for s = 0..3:
 *     for each block j:  xin   T_s x C_s    the block's input (residual stream)
 *                        qkv   T_s x 3 C_s  q | k | v of LayerNorm(xin)
 *                        xmid  T_s x C_s    xin + o_proj(window attention)
 *     m_s (s < 3)        T_s/4 x 4 C_s      the stage's output gathered 2 x 2 (= T_s C_s elements), before the merge LayerNorm
 *   xf                       49 x 768       the last block's output
 *   hnf                      49 x 768       final LayerNorm of xf
 * 8 053 248 elements per crop. */
int m2t_swin_encode_ex(m2t_swin* p, const float* src_a, int n_a, const float* src_b, int n_b, int Hs, int Ws,
                       const int* crops_host, int n, float* emb, void* workspace, void* stream, void* hidden_out);

/* m2t_swin_backward with observation points (m2t_swin_backward is this call with grad_taps = NULL; same kernels, same g_crops
 * bits).  grad_taps (device fp32, may be NULL) receives the residual-stream gradient of the n_grad crops, one after the other
 * in backward order, each [n_grad][elements per crop]:
 *   after the final LayerNorm backward                                   49 x 768   (gradient w.r.t. xf)
 *   for s = 3..0:
 *     for each block j, last to first:  after the MLP half               T_s x C_s  (gradient w.r.t. xmid)
 *                                       after the attention half         T_s x C_s  (gradient w.r.t. xin)
 *     after the merge scatter (s > 0)                                    T_{s-1} x C_{s-1}  (gradient w.r.t. stage s - 1's output)
 *   after the embedding LayerNorm backward                               3136 x 96  (gradient w.r.t. e0)
 * 3 725 568 floats per crop.  g_crops is the last stage's output, as in the plain call. */
int m2t_swin_backward_ex(m2t_swin* p, const float* g_emb, int n_grad, float* g_crops, void* workspace, void* grad_ws, void* stream,
                         float* grad_taps);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
