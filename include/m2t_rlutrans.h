/* m2t_rlutrans.h -- the training entry points of the util/rlutrans.py TransBlock of libm2t.so: a forward that keeps
 * what the backward reads, and the backward (data and parameter gradients), in HIP.
 *
 * An eighth header on the same library, under the conventions of m2t.h (extern "C", raw device pointers, a hipStream_t passed as
 * void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the seven older headers are unchanged and
 * m2t_transblock_forward / m2t_transblock_workspace_bytes of m2t.h stay the inference route.  Every entry only launches: no
 * allocation, no upload, no host synchronisation; they may sit inside a stream capture.
 *
 * params / gparams: the 22 928 fp32 values of TransBlock(n_feat=64, dim=64) in state_dict order (atten.reduce.weight [64,64],
 * atten.qkv.weight [192,64], atten.proj.weight [64,64], atten.proj.bias, norm1.weight, norm1.bias, mlp.fc1.weight [16,64],
 * mlp.fc1.bias, mlp.fc2.weight [64,16], mlp.fc2.bias, norm2.weight, norm2.bias).  x, y, gy, gx: [B,N,64] fp32, contiguous.
 * dtype: M2T_F32 (fp32 throughout) or M2T_BF16 (bf16 operands, fp32 accumulation; the residual-stream gradient stays fp32).
 *
 * Arithmetic of the backward: every reduction over tokens is two-stage in a fixed order with fp32 accumulation, there are no atomics,
 * every output element is written by exactly one thread: two runs are bit-identical, and nothing depends on what the workspace held
 * before m2t_transblock_forward_train. */
#ifndef M2T_RLUTRANS_H
#define M2T_RLUTRANS_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Bytes of the training workspace for [B,N,64]: the saved tensors of the forward, then the scratch of the backward.  No
 * initialisation needed.  0 for B < 1, N < 16 or an unknown dtype. */
size_t m2t_transblock_train_workspace_bytes(int B, int N, int dtype);

/* Where a region of that workspace starts (bytes), for audits and tests; (size_t)-1 for a bad shape or an unknown region.  All of
 * these are in the compute element type (float or bf16) and are written by m2t_transblock_forward_train only:
 *   0: H1 [M][16], the hidden units after the ReLU        1: AO [M][64], the attention output before proj
 *   2: the packed weights (the 22 928 values, then the transposes fc1^T [64][16], proj^T [64][64], qkv^T [64][192], reduce^T [64][64])
 *   3: X [M][64]    4: LN1(X) [M][64]    5: R [M][64], the reduce output    6: QKV [M][192]    7: X1 [M][64]    8: LN2(X1) [M][64]
 * with M = B * N. */
size_t m2t_transblock_train_workspace_offset(int B, int N, int dtype, int region);

/* The forward of m2t_transblock_forward -- the same kernels in the same order, so y is the same bit for bit -- keeping every tensor
 * the backward reads in `workspace` (m2t_transblock_train_workspace_bytes bytes).
 * M2T_ERR_ARG before any launch: a null argument, dtype other than M2T_F32 / M2T_BF16, B < 1, N < 16. */
int m2t_transblock_forward_train(const float* params, const float* x, float* y, int B, int N, int dtype, void* workspace, void* stream);

/* The backward of the forward_train call that last wrote `workspace` (same params, B, N, dtype): gx = d<gy, y>/dx and
 * gparams = d<gy, y>/dparams, both STORED (not added to).  Either of gx / gparams may be NULL, not both: with gparams NULL no weight,
 * bias or LayerNorm-affine reduction is launched; with gx NULL the data gradient of the first LayerNorm is not launched.  Only the
 * scratch part of the workspace is written, so the call may be repeated on one forward.
 * M2T_ERR_ARG before any launch: null params / gy / workspace, gx and gparams both NULL, a bad dtype, B < 1, N < 16. */
int m2t_transblock_backward(const float* params, const float* gy, float* gx, float* gparams, int B, int N, int dtype, void* workspace,
                            void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
