/* m2t_groups.h -- parameter groups and frozen ranges for the optimizer end of libm2t.so, in HIP.
 *
 * A sixth header on the same library, under the conventions of m2t.h and the four headers after it (extern "C", raw device pointers, a
 * hipStream_t passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the five older headers
 * are unchanged.  The two launching entries only launch: no allocation, no upload, no host synchronisation; they may sit inside a
 * stream capture.  The two table entries are pure host functions.
 *
 * What it replaces: torch.optim.Adam([{"params": ..., "lr": ..., "weight_decay": ...}, ...]) over a model part of whose parameters
 * have requires_grad = False, and torch.nn.utils.clip_grad_norm_ over the parameters that have a gradient.
 *
 * The SEGMENT TABLE describes the flat fp32 buffer of n elements: n_seg contiguous segments that cover [0, n) exactly, in ascending
 * order, none empty; segment i is [starts[i], starts[i + 1]) and belongs to group group[i] in 0 .. n_groups - 1.  Boundaries may fall
 * on any element.  The caller packs the table on the host ONCE, copies the blob to the device ONCE and hands the device pointer to
 * every step.  What changes from step to step -- each group's learning rate, weight decay and frozen flag -- travels BY VALUE with
 * the launch (host arrays of n_groups entries, read before the entry returns).
 *
 * Blob layout (8-byte aligned): long long {n_seg, n_groups, n, 0}; long long starts[n_seg + 1]; unsigned char group[n_seg]; padding
 * to a multiple of 8.  A kernel that finds another (n_seg, n_groups, n) in the blob than the launch was given returns without
 * reading or writing anything else: the table belongs to another buffer. */
#ifndef M2T_GROUPS_H
#define M2T_GROUPS_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define M2T_MAX_GROUPS 8
#define M2T_MAX_SEGMENTS 1024

/* Bytes of the packed table of n_seg segments; 0 for n_seg outside 1 .. M2T_MAX_SEGMENTS. */
size_t m2t_group_table_bytes(int n_seg);

/* Validate a table on the host and write its blob.  starts: n_seg + 1 values, starts[0] = 0, strictly ascending, starts[n_seg] = n;
 * group: n_seg ids in 0 .. n_groups - 1 (a group may own no segment).  blob_host: m2t_group_table_bytes(n_seg) bytes of HOST memory;
 * the caller copies them to the device.  M2T_ERR_ARG, with blob_host untouched: a null argument, n < 1, n_seg outside
 * 1 .. M2T_MAX_SEGMENTS, n_groups outside 1 .. M2T_MAX_GROUPS, a first start other than 0, starts that are not strictly ascending (an
 * unsorted table, an empty segment), a last bound other than n (a gap at the end, a table that falls short of or runs past n), an id
 * outside 0 .. n_groups - 1. */
int m2t_group_table_pack(const long long* starts_host, const int* group_host, int n_seg, long long n, int n_groups, void* blob_host);

/* m2t_adam_step_ex (m2t.h) with one (lr, weight_decay) per group and frozen groups: ONE launch over params, grads, exp_avg,
 * exp_avg_sq (+ ema).  lr, weight_decay: HOST arrays of n_groups floats; frozen: HOST array of n_groups bytes (non-zero = frozen).
 * table: the DEVICE copy of the blob packed for this n, n_seg and n_groups.  beta1, beta2, eps, step, grad_scale, ema (may be NULL),
 * decoupled, ema_decay and record (may be NULL) are m2t_adam_step_ex's and are shared by every group.
 * Every element of a group that is not frozen goes through exactly the fp32 operation sequence of m2t_adam_step_ex called with that
 * group's lr and weight_decay (pmul = float32(1 - lr * weight_decay) is formed on the host in fp64, per group; a group whose weight
 * decay is 0 takes neither decay branch, as there): the result is bit-identical to m2t_adam_step_ex on the group's slices.
 * An element of a FROZEN group is neither read nor written: params, exp_avg, exp_avg_sq and ema keep every bit and grads is not
 * loaded there, so what a frozen range of grads holds (stale values, NaN) is immaterial.  With record != NULL and applied == 0 in
 * it nothing is written at all.  grads is read only.
 * A 16-byte vector whose four elements lie in one segment is one vector load / store per buffer; a vector that straddles a segment
 * boundary and the last n % 4 elements are handled element by element.
 * M2T_ERR_ARG before any launch: n < 1, a null params / grads / exp_avg / exp_avg_sq / lr / weight_decay / frozen / table, a buffer
 * that is not 16-byte aligned, step < 1, ema_decay outside [0, 1), n_groups outside 1 .. M2T_MAX_GROUPS, n_seg outside
 * 1 .. min(n, M2T_MAX_SEGMENTS), a negative or NaN weight decay, a NaN learning rate. */
int m2t_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, const float* lr_host,
                         float beta1, float beta2, float eps, int step, float grad_scale, float* ema,
                         const float* weight_decay_host, int decoupled, float ema_decay, const double* record,
                         const unsigned char* frozen_host, int n_groups, const void* table, int n_seg, void* stream);

/* m2t_grad_norm (m2t.h) over the elements of the groups that are not frozen: clip_grad_norm_ over the parameters that have a
 * gradient.  The same fixed grid, the same element -> accumulator mapping and summation order, the same second stage, the same
 * workspace size (m2t_grad_norm_workspace_bytes) and the same record layout.  Defined result: the record is BIT-IDENTICAL to the one
 * m2t_grad_norm writes for a copy of grads whose frozen ranges hold +0.0.  A frozen element is never loaded: a NaN or Inf there
 * changes no bit of the record and never triggers the non-finite skip.  grads needs 4-byte alignment only, as there.
 * M2T_ERR_ARG before any launch: n < 1, a null grads / record / workspace / frozen / table, step < 1, a NaN max_norm, n_groups
 * outside 1 .. M2T_MAX_GROUPS, n_seg outside 1 .. min(n, M2T_MAX_SEGMENTS). */
int m2t_grad_norm_groups(const float* grads, long long n, float grad_scale, float max_norm, int skip_nonfinite, int step, float beta1,
                         float beta2, double* record, void* workspace, const unsigned char* frozen_host, int n_groups,
                         const void* table, int n_seg, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
