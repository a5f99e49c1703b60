/* m2t.h -- C ABI of libm2t.so: the MI355X (gfx950) implementation of the M2Trans
 * data-parallel training-step hot path.
 *
 * The reference (eezkni/M2Trans) has no FFI: its hot path sits behind a Python plugin hook,
 *     utils.import_module('models.M2Trans_network').create_model(args)      (train.py:70)
 *     sr = model(lr)                                                         (train.py:183)
 *     loss = L1Loss()(sr, hr) * lambda_l1 ; loss.backward() ; optimizer.step() (train.py:199-210)
 * This library is what a drop-in `models/M2Trans_network.py` binds with ctypes
 * (m2trans_amd/M2Trans_network.py; the binding a maintainer adds is shown in INTEGRATION.md).
 * Every entry point takes plain device pointers, sizes and a hipStream_t; no torch types.
 *
 * Conventions
 *   - return 0 on success, < 0 for argument errors (m2t_status), > 0 = hipError_t of a failed
 *     launch; m2t_last_error_string() describes the last failure on the calling thread.
 *     (The reference raises Python exceptions: `assert` M2Trans_network.py:305, ValueError
 *     train.py:72, RuntimeError/KeyError M2Trans_network.py:100-112.)
 *   - kernels never allocate, free or synchronise; the caller owns every buffer, including the
 *     workspace whose size the plan reports.  All launches go to the given stream, so the whole
 *     step can be captured in a HIP graph.
 *   - tensors at the boundary use the reference's layout: NCHW float32, values in [0, rgb_range].
 *     Internal activations are NHWC in `dtype` (0 = float32, exact-fp32 MFMA; 1 = bfloat16 MFMA
 *     with fp32 accumulation / statistics / softmax / master weights).
 *   - parameters live in ONE flat float32 buffer, the trainable tensors of the reference's
 *     state_dict in registration order (head.weight, head.bias, body.0.attn1.rel_h, ...,
 *     tail.*; the 4 frozen MeanShift tensors are not part of it -- they are never used by
 *     forward, M2Trans_network.py:30-31,58-76).  Gradients use the same layout, which is what
 *     makes the data-parallel exchange a single RCCL all-reduce.
 */
#ifndef M2T_H
#define M2T_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#pragma GCC visibility push(default)

typedef struct m2t_plan m2t_plan;

enum m2t_status { M2T_OK = 0, M2T_ERR_ARG = -2, M2T_ERR_STATE = -3 };

int m2t_version(void);
const char* m2t_last_error_string(void);

/* ---- plan: shapes, parameter offsets, workspace layout -------------------------------- */
/* replaces M2Trans.__init__ (models/M2Trans_network.py:17-56) for fixed n_feats = 64, colors = 3.
 * (B, H0, W0) = LR batch shape; the image is reflect-padded to multiples of 32 internally
 * (check_image_size, :78-86). scale in {2,3,4}. */
int m2t_plan_create(m2t_plan** out, int B, int H0, int W0, int scale, int n_blocks, int dtype);
void m2t_plan_destroy(m2t_plan* p);
/* named integer queries: "workspace_bytes", "num_params", "padded_h", "padded_w",
 * "param:<state_dict name>" (offset in floats), "numel:<state_dict name>",
 * "ws:<tensor>" (byte offset of a workspace tensor, e.g. "ws:b0.qkv3"), "wsn:<tensor>" (elements).
 * Returns -1 for an unknown key. */
long long m2t_plan_query(const m2t_plan* p, const char* key);
/* Scheduling / kernel-selection options: each selects between a fused gfx950 kernel and the plain kernels it replaces
 * (which fp32 parity mode always uses), or places the parameter-gradient work; results are the same up to bf16 rounding and
 * every pair is A/B-tested in tests/test_gpu_model.py.  Defaults in brackets; m2t_plan_query("opt:<key>") reads the value in
 * force (gate_branch / wgrad_big_tiles are reported + 1000).  Variants that were measured and lost live under scratch/ with
 * their numbers in profiles/README.md, not behind options.
 *   "side_stream"       [1] parameter-gradient kernels of m2t_backward on a plan-owned second stream; 0 enqueues the same kernels with
 *                           the same arguments in the same order on the caller's stream, so both settings give BIT-IDENTICAL losses,
 *                           gradients and input gradients at every step (no kernel of the step uses atomics): enforced by
 *                           tests/test_gpu_schedule.py, where any difference is a missing stream dependency
 *   "gate_branch"       [-1] -1: a branch's side work is released right behind its attention launch; 0..3: a block's side work waits for the
 *                           attention launch of that branch (2 = behind the two LDS-filling C = 256 launches; the default of rounds 1-2,
 *                           when the main chain still waited for the side stream once per branch)
 *   "fork_on_kernel"    [1] the event that releases side-stream work rides on the main-stream dispatch it follows (hipExtLaunchKernelGGL
 *                           stop event) instead of a marker packet behind it: -0.7 % step time; 0 = hipEventRecord.  Ignored (0) while the
 *                           stream is being captured into a HIP graph
 *   "fused_prep_fwd"    [1] bf16, C = 64 / 256 branches: branch_prep (norm apply + branch mixing + DWT^L) inside the fused forward attention kernel
 *                           (needs "fused_attn_fwd" >= 1; bit-identical); 0 = branch_prep launches in front of it
 *   "fused_prep_bwd"    [1] bf16: the backward of branch 4's branch_prep inside branch 3's attention backward (same level and window grid; needs
 *                           "attn_bwd" >= 2; bit-identical); 0 = a branch_prep_bwd launch between the two
 *   "fused_l1"          [1] bf16 x4 with the recomputing fused tail backward ("fused_tail" = 2 / 3): a loss requested through m2t_l1_loss_deferred
 *                           is taken inside that kernel (clamp, |sr - hr| partial sums, sign seed on the staged halo); 0 = m2t_backward runs the
 *                           clamp + L1 kernel first (bit-identical gradients either way)
 *   "tail_bwd_mfma32"   [1] bf16 x4 with the recomputing fused tail backward ("fused_tail" = 2 / 3): the round-6 form of that kernel on
 *                           v_mfma_f32_32x32x16_bf16 (k_tail_bwd.hip: LDS pixel order by sub-pixel position, conflict-free operand reads with half
 *                           the bytes per FLOP, gelu'(t2) and g(t2) formed in registers, reflect-border gather without divergent loops, three
 *                           barriers per tile): 346 us against 426 us stand-alone at batch 16.  g(t1), dW3 bit-identical to the 16x16x32 kernel
 *                           (0), dWf / db3 the same products in another fp32 order
 *   "fp32_fast"         [1] fp32: the round-5 kernels of the parity mode -- plain GEMMs (qkv projections and their data gradients, N % 32 == 0,
 *                           K % 32 == 0), qkv weight gradients (N % 64 == 0, K % 64 == 0), the x2 expansions 64 -> 256 (image rows of whole
 *                           128-pixel tiles) and their weight / bias gradients on v_mfma_f32_32x32x2_f32 (k_gemm.hip), the 64 -> 3 tail conv
 *                           weight and data gradient on the VALU (k_conv.hip): exact fp32 products, fp32 accumulation, other summation orders;
 *                           0 = the 16x16x4 kernels of rounds 1-4
 *   "fused_attn_fwd2"   [0] bf16, C = 256 branches with "fused_prep_fwd": the forward kernels that put TWO windows on a CU (k_attn_fwd2.hip: projection
 *                           in four output-channel chunks, scores / softmax / P in registers, v re-read from L2 for P V, IWT^2 straight from the
 *                           accumulators): 1 = 4-wave workgroups of one window (80 KB of LDS, two per CU), 2 = 8-wave workgroups of two
 *                           neighbouring windows (1 for an odd number of windows per image), -1 = variant 1 when the branch has more windows than
 *                           the chip has CUs (batch >= 17 at 128 x 128), 0 = never.  q | k | v bit-identical to the one-window-per-CU kernel, the
 *                           output to fp32 summation order.  Measured at batch 32: 59.3 us against 61.7 us stand-alone, a tie inside the step (both
 *                           windows of a CU start together and stay in the same phase: there is nothing for co-residency to overlap): off by default
 *   "fused_norm_red"    [0] bf16 with "attn_bwd" = 3: the first reduction stage of the InstanceNorm backward (sums of g_n and g_n * xhat per image
 *                           and channel) rides in the C = 16 prep launch -- extra workgroups for the planes of branches 2 .. 4, per-tile sums of
 *                           plane 0 from the tiles that produce it; 0 = its own launch behind that kernel (same sums, another addition order).
 *                           Measured 2.2 % SLOWER on the step (round 5: both roles are memory-heavy and do not overlap): off by default
 *   "wgrad_big_tiles"   [-1] qkv weight gradient of the C = 256 branches with 128 x 128 output tiles: value = target number of
 *                           workgroups (64..512), 0 = off, -1 = auto (256 from 24 576 branch pixels on, i.e. batch >= 24)
 *   "fused_tail"        [3] bf16 x4: 1 = one fused kernel for the high-resolution half of the tail backward (k_tail_bwd.hip); 2 = the same
 *                           and tail.3 expansion + PixelShuffle + GELU + tail conv of the FORWARD in one kernel (k_tail_fwd.hip): gelu(t2)
 *                           and gelu'(t2) are then never stored, the fused backward recomputes them per tile
 *                           (m2t_plan_query("stores_t2") tells whether ws:t2act / ws:t2der are written); 3 = 2 with the forward as the
 *                           row-streaming kernel of round 4 (k_tail_stream.hip, same bits); 4 = 3 with the backward as a row-streaming
 *                           kernel too (k_tail_bwd_stream.hip: same data gradient bits, slower -- kept for A/B); 0 = the plain kernels.
 *                           bf16 x2 / x3: >= 1 = the whole tail as ONE row-streaming forward and ONE recomputing backward kernel
 *                           (m2t_plan_query("stores_t1") = 0: gelu(t) / gelu'(t) are never stored), 0 = the plain kernels
 *   "attn_bwd"          [3] bf16 attention backward: 0 = chunked kernels + halo gather + data-gradient GEMM, 1 = whole-window-
 *                           resident / wave-per-window kernels, 2 = 1 + the data gradient of the qkv projection inside the
 *                           C = 64 / 256 kernels (k_attn_res.hip), 3 = 2 + one kernel for the C = 16 branch's overlap-add,
 *                           projection data gradient and branch_prep_bwd (k_attn_c16.hip; bit-identical to 2)
 *   "conv_rows"         [1] bf16 conv3x3 64 -> 64 (forward and data gradient): row-streaming kernel fed by LDS-DMA with the weights in
 *                           registers (k_conv.hip); 0 = the 8 x 16 tile kernel it replaced (also the fallback for widths the strip
 *                           geometry does not divide).  Bit-identical
 *   "fused_conv_bwd"    [1] bf16 conv3x3 64 -> 64 backward: data gradient and weight / bias gradient in ONE row-streaming pass over the
 *                           output gradient on the main stream (k_conv.hip; data gradient bit-identical, weight gradient the same
 *                           products summed in a different order); 0 = data gradient kernel + weight-gradient kernel on the side stream
 *   "fused_attn_fwd"    [2] bf16, C = 64 / 256: 1 = qkv projection + window attention + IWT / residual in one kernel per window; 2 = the
 *                           same and q | k | v of the C = 64 branch are NOT stored: the resident backward recomputes them from the
 *                           branch input (identical bits; needs "attn_bwd" = 2; m2t_plan_query("stores_qkv2")); 0 = GEMM + attention
 *   "fused_c16_fwd"     [2] bf16, C = 16: 1 = InstanceNorm apply + qkv projection + window attention + residual in one kernel, one wave per
 *                           window; 2 = the same and q | k | v of that branch are NOT stored: the backward kernel recomputes them from
 *                           the branch input (identical bits; needs "attn_bwd" >= 1; m2t_plan_query("stores_qkv1") tells whether
 *                           ws:b*.qkv1 is written); 0 = three kernels
 *   "debug_skip_side"   [0] timing experiments only: skips every parameter-gradient kernel (results are WRONG)
 *   "inference"         [0] 1 = an INFERENCE PLAN: m2t_forward alone, on a forward-only workspace.  "workspace_bytes", "ws:<name>" and
 *                           "wsn:<name>" then describe a layout resolved from the options in force when they are asked: the persistent regions
 *                           and X0 as before, X1 .. X<n_blocks> alternating between two buffers, ONE set of per-block regions that every
 *                           "b<k>." name resolves to, and no region the forward never reads -- q | k | v on the fused attention paths, the tail's
 *                           gelu' tensors, every backward region and the reduction arena answer -1 and the kernels get a null pointer for
 *                           them.  The same kernels in the same order as a training plan's forward: sr is BIT-IDENTICAL.  May be set or
 *                           cleared only before the first m2t_plan_init_workspace; on an initialised inference plan every other
 *                           m2t_set_option is M2T_ERR_STATE (the layout is frozen), as are m2t_forward with keep_activations != 0, every
 *                           plan-taking loss entry, m2t_set_output_grad / m2t_add_output_grad, m2t_backward / m2t_backward_ex and
 *                           m2t_stream_wait_bucket: an inference forward leaves neither activations nor a seed
 *   "local_norm"        [0] 0 = off; 8 .. 16384 = T: LOCAL-WINDOW InstanceNorm statistics (the Test-time Local Converter of Chu et al.,
 *                           ECCV 2022): every CFTM block normalises each pixel with the statistics of a T x T window around it instead
 *                           of the whole plane's.  Anything else is M2T_ERR_ARG.  Legal only on a plan whose "inference" is already 1 and
 *                           only before the first m2t_plan_init_workspace (else M2T_ERR_STATE, the text says which rule); clearing
 *                           "inference" while "local_norm" > 0 is M2T_ERR_STATE.  Definition, for a block input X on the padded plane
 *                           H x W (multiples of 32) and per axis k = min(T, side):
 *                             - the window of output row y is rows [i, i + k_h), i = clamp(y - (k_h - 1) / 2, 0, H - k_h), integer
 *                               division; columns likewise.  This is TLC's integral-image average: a left pad of (k - 1) / 2, a right pad
 *                               of k / 2, replicated edges.  Every window is full: the count is n = k_h k_w everywhere.
 *                             - per image, channel and pixel: S1 = sum x and S2 = sum x^2 over the window, in fp64 from the stored X
 *                               (plan dtype); m = S1 / n; v = max(S2 / n - m^2, 0); r = 1 / sqrt(v + 1e-5) (biased variance,
 *                               InstanceNorm2d's eps), all in fp64.
 *                             - mean32 = fl32(m), rstd32 = fl32(r); xn = round_to_plan_dtype((fl32(x) - mean32) * rstd32), the
 *                               subtraction and the product as separate fp32 operations.
 *                           T >= max(H, W) is the global InstanceNorm over the plane, in this arithmetic.  (Parity with the TLC code
 *                           itself is unpinned.)  Per block: statistics + apply -> "ws:xn" (through the fp64 sums "ws:lnsum"), then the
 *                           forward's launches in their order on xn with the identity record "ws:norm_id" (mean = 0 then rstd = 1, [B][64]
 *                           floats each); the 3 x 3 conv keeps the un-normalised X as its residual and emits no statistics partials.
 *                           The three regions answer -1 while the option is 0, and then every plan is laid out and launched as before.
 *                           The last block's input stays in place: "ws:X<n_blocks - 1>"
 *   "health"            [0] the STEP HEALTH RECORD of a training plan: 0 = off (the plan is laid out and launched as before: the same
 *                           "workspace_bytes", the same launches, the same bits; "ws:health" answers -1), 1 = a record of the tensors
 *                           m2t_forward stores, 2 = level 1 and the tensors m2t_backward / m2t_backward_ex leave.  Any other value is
 *                           M2T_ERR_ARG.  Set only before the first m2t_plan_init_workspace (after it: M2T_ERR_STATE) and only on a
 *                           training plan (on a plan whose "inference" is 1: M2T_ERR_STATE; setting "inference" to 1 while "health" > 0
 *                           is M2T_ERR_STATE too); each refusal's text names its rule.  The workspace gains "ws:health", double
 *                           [1 + rows][72], "ws:health_part" (the per-chunk partials) and two tables, all written by
 *                           m2t_plan_init_workspace, which zeroes the record.  ROWS, fixed from the layout table and the options in
 *                           force: "sr" (the caller's output, fp32 [B,3,Hs,Ws]; empty when sr == NULL); the regions the forward writes, in
 *                           its order -- X0, then per block b<k>.mean, .rstd, .d1, .qkv1 .. .d4, .qkv4, .xc, X<k + 1>, then t1act, t1der,
 *                           t2act, t2der, srpre; at level 2 the regions the backward leaves -- g_t2pre, g_t1pre, gT, gA, gB (g(X<k>) of
 *                           the even / odd blocks k >= 1), gqkv0 .. gqkv3, gqkv0b .. gqkv3b (dq | dK | dV of the last even / odd block), gn,
 *                           gxc (after block 0: the head's cotangent g(res)) -- and last "grads", the caller's flat gradient buffer
 *                           (all of it behind an all-stages pass; empty behind a pass with a stage flag clear, which also leaves the
 *                           regions it does not write as they were).  A tensor the options in force do not store has NO row: q | k | v
 *                           of the recomputing attention paths, the GELU tensors of the fused tails, g_t1pre / g_t2pre of the fused tail
 *                           backwards; clear that option to look inside.  On an initialised plan with "health" > 0 the options that
 *                           decide what is stored ("fused_tail", "attn_bwd", "fused_attn_fwd", "fused_c16_fwd") are M2T_ERR_STATE.
 *                           m2t_plan_query: "health_rows"; "health_row:<name>" = index or -1 (<name>: "sr", "grads" or a "ws:" name);
 *                           "health_phase:<index>" = 0 forward / 1 backward; "health_name:<index>" = the length of the row's name,
 *                           which it leaves where m2t_last_error_string() reads.
 *                           ROW r = ws:health[1 + r][0 .. 71] over the region's stored elements (padding counts: it is stored data),
 *                           each widened to fp32 exactly, then to fp64:
 *                             [0] n   [1] non-finite elements (NaN, +-Inf)   [2] NaNs   [3] max |x| over finite elements (0: none)
 *                             [4] sum and [5] sum of squares over finite elements   [6] exact zeros (+-0)
 *                             [7] min |x| over finite non-zero elements (+Inf: none)
 *                             [8 + k], k = 0 .. 63: exponent histogram -- bin 0 zeros; bins 1 .. 62 the finite non-zero elements with
 *                             clamp(floor(log2 |x|), -41, 20) + 42, from the fp32 bit pattern (subnormals: bin 1); bin 63 non-finite
 *                           HEADER ws:health[0]: [0] forward passes recorded, [1] backward passes recorded, [2] the first row, in row
 *                           order, of the last recorded forward with [1] > 0, or -1, [3] the same for the last recorded backward among
 *                           the backward rows, [4] rows, zeros beyond.  Counts, max, min and histogram are exact; the sums are fp64,
 *                           folded in an order the element index alone fixes: chunks of 32768 elements, inside a chunk 256 lanes taking
 *                           groups of 8 elements round-robin, the lanes by a halving tree, the chunks of a row in ascending order
 *                           (csrc/m2t_health_tile.h).  Bit-reproducible, no atomics, no allocation, no host synchronisation; two
 *                           launches behind the forward's last kernel, two on the main stream behind the backward's join of the side
 *                           stream (both schedules); the kernels write the two regions only
 *   "health_on"         [1] the run-time switch of the record: 0 = the passes skip its launches (the record and its pass counters
 *                           stay as they are).  Any time on a training plan, no effect while "health" is 0; M2T_ERR_STATE on an
 *                           inference plan, M2T_ERR_ARG beyond 0 / 1 */
int m2t_set_option(m2t_plan* p, const char* key, long long value);
/* Gradient buckets for communication overlap (replaces the reduce-to-GPU-0 of nn.DataParallel, train.py:73):
 * m2t_backward completes the flat gradient buffer in "grad_buckets" contiguous ranges, in this order: tail, block
 * pairs from the last to the first, head.  m2t_plan_query("grad_bucket_lo:<i>" / "grad_bucket_hi:<i>") give bucket
 * i's float range; after m2t_backward has been ENQUEUED, m2t_stream_wait_bucket makes `stream` wait until bucket i
 * is final, so an all-reduce of that range can run under the rest of the backward pass.  After an m2t_backward_ex pass with
 * some stage flag clear, every bucket event marks the end of that whole pass. */
int m2t_stream_wait_bucket(m2t_plan* p, int bucket, void* stream);
/* Initialisation of the workspace (uploads the weight-packing tables, clears the zero page); synchronises `stream`.
 * Four workspace regions PERSIST across steps and must not be overwritten by the caller: "zero_page" (zeros), "pack_descs" and
 * "pack_blocks" (the weight-packing tables), all three written here, and "red_descs" (the table of the deferred gradient
 * reductions), written by the first all-stages m2t_backward after this call.  Every other region is scratch WITHIN one step: each
 * m2t_forward / m2t_backward writes whatever it reads before it reads it, so the contents left by an earlier step (or by the
 * allocator) never reach a result -- tests/test_gpu_schedule.py fills them with NaN between steps.  (An inference plan has the first
 * three persistent regions and no "red_descs"; the same contract holds for its aliased layout: tests/test_gpu_lean_inference.py.
 * With option "local_norm" > 0 it has a fourth, "norm_id", written here: tests/test_gpu_local_norm.py.)
 * Calling this again on a live plan is legal (with the same or another buffer, once the plan's earlier work on `stream` is
 * enqueued): it returns the plan to "no activations, no seed", and the next all-stages backward publishes "red_descs" again. */
int m2t_plan_init_workspace(m2t_plan* p, void* workspace, void* stream);

/* ---- model ----------------------------------------------------------------------------- */
/* M2Trans.forward (models/M2Trans_network.py:58-76): x [B,3,H0,W0] -> sr [B,3,H0*s,W0*s].
 * keep_activations: a training plan keeps everything m2t_backward needs whatever the argument says; an inference plan (option
 * "inference") keeps nothing, and a non-zero argument is M2T_ERR_STATE there. */
int m2t_forward(m2t_plan* p, const float* params, const float* x, float* sr, float rgb_range,
                int keep_activations, void* workspace, void* stream);
/* L1Loss()(sr, hr) * lambda_l1 (train.py:76,199) on the forward's output + the backward seed.
 * loss_out: device float[1].  divisor = number of elements the mean runs over (pass the GLOBAL
 * count B_global*3*Hs*Ws under data parallelism so that SUM-all-reduced gradients equal the
 * full-batch gradient). */
int m2t_l1_loss(m2t_plan* p, const float* hr, float lambda_l1, double divisor, float rgb_range,
                float* loss_out, void* workspace, void* stream);
/* The same loss and seed, produced INSIDE the next m2t_backward (round 5): loss_out is valid in stream order behind that call, and
 * hr must stay valid until it has been issued.  On the bf16 x4 path the fused tail backward takes the clamp + L1 seed while it
 * stages its g(sr) halo (option "fused_l1"): the seed tensor is never written, one 150 MB pass and two launches leave the step;
 * on every other path m2t_backward runs m2t_l1_loss's kernel first (identical results to m2t_l1_loss).  The loss value differs
 * from m2t_l1_loss's by the order of an fp32 sum.  A later m2t_l1_loss / m2t_set_output_grad / m2t_forward cancels it. */
int m2t_l1_loss_deferred(m2t_plan* p, const float* hr, float lambda_l1, double divisor, float rgb_range,
                         float* loss_out, void* workspace, void* stream);
/* The pixel-loss family: weight * mean(rho(clamp(sr) - hr)) + the backward seed, for the criteria the reference offers next to L1
 * (losses.py:225-230: l1 / sl1 = nn.SmoothL1Loss / l2 = nn.MSELoss; losses.py:287-297: L1_Charbonnier_loss, eps added under the
 * root as in :295).  With d = clamp(sr) - hr, in fp32:
 *   M2T_LOSS_L1           |d|                                               seed factor sign(d) (0 at d = 0)      param unused
 *   M2T_LOSS_MSE          d^2                                               2 d                                   param unused
 *   M2T_LOSS_CHARBONNIER  sqrt(d^2 + eps)                                   d / sqrt(d^2 + eps)                   param = eps  (1e-6 in the reference)
 *   M2T_LOSS_SMOOTH_L1    |d| < beta ? d^2 / (2 beta) : |d| - beta / 2      |d| < beta ? d / beta : sign(d)       param = beta (1.0 in torch)
 * seed = factor * (float)(weight / divisor) where 0 <= pre-clamp output <= rgb_range inside the image, 0 elsewhere.
 * m2t_pixel_loss is m2t_l1_loss, m2t_pixel_loss_deferred is m2t_l1_loss_deferred with the kind chosen: the same state rules, the same
 * launches, the same schedule ("fused_l1" takes EVERY kind inside the fused tail backward on the bf16 x4 path; on every other path
 * m2t_backward runs m2t_pixel_loss's kernel first), and a later loss / m2t_set_output_grad / m2t_forward cancels a deferred request.
 * kind = M2T_LOSS_L1 is m2t_l1_loss / m2t_l1_loss_deferred, bit for bit.  m2t_add_output_grad works on the seed of any kind.
 * M2T_ERR_ARG: an unknown kind; eps / beta not finite or not > 0 (beta = 0 is the L1 loss: ask for M2T_LOSS_L1).
 * M2T_ERR_STATE: no forward with saved activations. */
enum m2t_pixel_loss_kind { M2T_LOSS_L1 = 0, M2T_LOSS_MSE = 1, M2T_LOSS_CHARBONNIER = 2, M2T_LOSS_SMOOTH_L1 = 3 };
int m2t_pixel_loss(m2t_plan* p, int kind, float param, const float* hr, float weight, double divisor, float rgb_range,
                   float* loss_out, void* workspace, void* stream);
int m2t_pixel_loss_deferred(m2t_plan* p, int kind, float param, const float* hr, float weight, double divisor, float rgb_range,
                            float* loss_out, void* workspace, void* stream);
/* alternative seed: an arbitrary upstream gradient g_sr [B,3,H0*s,W0*s] (torch autograd). */
int m2t_set_output_grad(m2t_plan* p, const float* g_sr, float rgb_range, void* workspace, void* stream);
/* adds scale * g into the seed already materialised by m2t_l1_loss / m2t_pixel_loss or m2t_set_output_grad (the opt-in differentiable
 * SemanticLoss): g [B,3,gh,gw] float32; sample b's block lands at crops_host int[B][2] = (row0, col0) of the SR image, or at
 * (0, 0) for every sample when crops_host is NULL; the same clamp mask and padded layout as m2t_set_output_grad.
 * M2T_ERR_STATE without a seed or after m2t_l1_loss_deferred / m2t_pixel_loss_deferred (no materialised seed); M2T_ERR_ARG for a block outside the image. */
int m2t_add_output_grad(m2t_plan* p, const float* g, int gh, int gw, const int* crops_host, float scale, float rgb_range,
                        void* workspace, void* stream);
/* The structural term of the loss surface: weight * (1 - mean SSIM) with its gradient (the reference's losses.py:8 imports SSIMLoss /
 * MultiScaleSSIMLoss from piq next to the pixel criteria; utils.py:232-234 scores every epoch by pytorch_msssim.ssim).  Per channel,
 * the pytorch_msssim.ssim / piq.ssim(downsample=False) form: x = clamp(pre, 0, R) / R, y = hr / R (data_range 1), separable 11-tap
 * Gaussian sigma 1.5 (the fp32 taps torch.exp / torch.sum give, as pytorch_msssim builds them, widened to fp64), VALID -> a (H-10) x (W-10) map per
 * channel, K = (0.01, 0.03), no non-negativity clamp.  Moments, map and gradient coefficients are fp64; inputs are fp32; every
 * gradient value is rounded to fp32 once and added in fp32.  Deterministic (no atomics; partial sums folded in a fixed order).
 * piq.SSIMLoss's default downsample=True (an average pooling in front, by 2 at 512 x 512) is NOT applied.  MS-SSIM is not offered.
 *
 * m2t_ssim_loss_tensor (plan-free): x [B,C,H,W] float32 on the device with image stride x_image_stride, channel stride
 * x_image_stride / C, row stride x_row_stride (elements); y contiguous [B,C,H,W].  With S the SSIM map of (x / data_range, y / data_range),
 * x clamped to [0, data_range] first when clamp != 0:
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum_map (1 - S))        (pass scale = 1 / map entries for the mean)
 *   gx_add[q]  += (float)(-scale * d sum(S) / dx[q])     x's strides; where clamp != 0 and x[q] is outside [0, data_range] (ends
 *                 included in the pass band) the element is left alone; elements outside [H,W] are never touched; NULL = value only.
 * scratch: m2t_ssim_loss_scratch_bytes(B, C, H, W) bytes on the device (0 when H < 11 or W < 11), no initialisation needed.
 * M2T_ERR_ARG: a null x / y / loss_out / scratch, H or W < 11, data_range not a finite number > 0, B * C outside 1 .. 65535, strides
 * that do not hold the image.
 *
 * m2t_ssim_loss: the same routine on the forward's pre-clamp output (rgb_range = R, the clamp on), adding into the seed that
 * m2t_l1_loss / m2t_pixel_loss (weight 0 for SSIM alone) or m2t_set_output_grad materialised: seed += -(weight / divisor) / R *
 * d sum(S) / dx through the clamp mask, exactly 0 in the reflect padding; loss_out as above with scale = weight / divisor.  divisor =
 * the GLOBAL number of map entries, world * accum * B * 3 * (Hs-10) * (Ws-10), so that rank shards and micro-batches sum to
 * weight * (1 - global mean SSIM) (the scheme of the pixel term).  scratch: m2t_ssim_loss_scratch_bytes(B, 3, Hs, Ws).
 * State rules of m2t_add_output_grad: M2T_ERR_STATE without a forward with saved activations, without a seed, or after
 * m2t_l1_loss_deferred / m2t_pixel_loss_deferred.  M2T_ERR_ARG: a null argument, an SR image below 11 x 11, a bad rgb_range / divisor. */
size_t m2t_ssim_loss_scratch_bytes(int B, int C, int H, int W);
int m2t_ssim_loss_tensor(const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride, int x_row_stride,
                         float data_range, int clamp, double scale, float* gx_add, float* loss_out, int accumulate, void* scratch,
                         void* stream);
int m2t_ssim_loss(m2t_plan* p, const float* hr, float weight, double divisor, float rgb_range, float* loss_out, int accumulate,
                  void* scratch, void* workspace, void* stream);
/* loss.backward() (train.py:209) restricted to the model: fills grads (flat, same layout as
 * params; every element is written). */
int m2t_backward(m2t_plan* p, const float* params, const float* x, float* grads, void* workspace,
                 void* stream);
/* m2t_backward with a choice of outputs (torch's requires_grad on the input and on whole stages of the model).
 * need_stage: host array of n_blocks + 2 flags in state_dict order -- [0] head, [1 + b] body.b, [n_blocks + 1] tail -- or NULL =
 * every stage.  A stage's contiguous range of grads is written iff its flag is set (other ranges are not touched); grads may be
 * NULL when no flag is set.  x is read only when the head's flag is set.  gx: NULL, or the gradient with respect to the input,
 * fp32 NCHW [B,3,H0,W0] (every element written; deterministic).  The data-gradient chain runs from the tail down to the lowest
 * stage that is needed, or to the input when gx != NULL.  need_stage = NULL and gx = NULL launch exactly what m2t_backward
 * launches.  A pass with some flag clear never changes the plan's reduction table (the first pass with a given set of flags
 * uploads a table of its own, so it cannot be captured into a graph; later ones can); after it, every gradient bucket event is
 * recorded at its end: m2t_stream_wait_bucket then waits for the whole pass.  No flag set: no side-stream work at all.
 * M2T_ERR_ARG: nothing requested (no flag, gx NULL), a flag set with grads NULL, the head's flag set with x NULL;
 * M2T_ERR_STATE: no forward with saved activations or no seed (the seed is consumed, as by m2t_backward). */
int m2t_backward_ex(m2t_plan* p, const float* params, const float* x, float* grads, float* gx,
                    const unsigned char* need_stage, void* workspace, void* stream);
/* torch.optim.Adam(lr, betas, eps, weight_decay=0).step() (train.py:81,210), fused over the flat
 * buffers; step = 1-based count; grad_scale multiplies g first (1/world_size after a SUM all-reduce). */
int m2t_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n,
                  float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/* Gradient accumulation over micro-batches (torch's AccumulateGrad under loss.backward() called several times before
 * optimizer.step(), train.py:209-210): acc[i] = acc[i] + g[i] for i in [0, n) -- ONE IEEE fp32 addition per element, no
 * scaling, no other arithmetic, so the result is the same bits as torch's acc += g.  acc and g: device pointers, 4-byte
 * aligned, not overlapping (any n >= 0; 16-byte loads and stores when both are misaligned to 16 bytes by the same amount, a
 * scalar loop otherwise).  loss_acc / loss_part: both NULL, or device float[1] each: loss_acc[0] = loss_acc[0] + loss_part[0]
 * in the same launch.  M2T_ERR_ARG: null acc / g with n > 0, n < 0, exactly one of the two loss pointers set. */
int m2t_grad_accumulate(float* acc, const float* g, long long n, float* loss_acc, const float* loss_part, void* stream);
/* The global gradient norm of the flat buffer and the decisions that hang on it (train.py:81,210 is the optimizer this feeds;
 * restates total = torch.nn.utils.clip_grad_norm_(params, max_norm), the torch.isfinite(total) test of a skipping loop, and
 * Adam's bias_correction1/2 for the step it will really take).  Two launches, no atomics: a fixed grid of fp64 partial sums of
 * (grad_scale * g)^2 into `workspace` (m2t_grad_norm_workspace_bytes() bytes, device, 8-byte aligned), then one workgroup that
 * adds them in index order and writes `record`: 8 doubles on the device, which the caller ZEROES once and then leaves alone --
 *   [0] norm = sqrt(sum)                      [1] finite = isfinite(norm)
 *   [2] clip_coef = min(1, max_norm / (float(norm) + 1e-6)) in fp32 as torch does; 1 when max_norm <= 0
 *   [3] applied = 0 when skip_nonfinite and the norm is not finite, else 1
 *   [4] skipped: running count of calls with applied == 0
 *   [5] 1 - beta1^t   [6] sqrt(1 - beta2^t)   [7] t = step - skipped: the bias correction of the EFFECTIVE step number
 * The summation tree depends on n (and the 16-byte phase of grads) alone: the same bits on every run and every device.
 * grads: device, 4-byte aligned, read only (any n >= 0).  The library allocates nothing and synchronises nothing.
 * M2T_ERR_ARG (decided on the host): n < 0, null grads with n > 0, null record or workspace, step < 1, NaN max_norm. */
int m2t_grad_norm(const float* grads, long long n, float grad_scale, float max_norm, int skip_nonfinite, int step,
                  float beta1, float beta2, double* record, void* workspace, void* stream);
long long m2t_grad_norm_workspace_bytes(void);
/* torch.optim.Adam(lr, betas, eps, weight_decay, decoupled_weight_decay).step() (train.py:81,210; the reference passes
 * weight_decay there) behind torch.nn.utils.clip_grad_norm_, with ema.mul_(d).add_(p, alpha=1 - d) in the same pass.  Arguments
 * up to grad_scale as m2t_adam_step.  Per element, fp32, in this order:
 *   g' = g * grad_scale * clip_coef;  coupled (decoupled == 0, weight_decay > 0): g' = g' + weight_decay * p;
 *   decoupled (AdamW): p = p * float32(1 - lr * weight_decay);  m, v, p as m2t_adam_step with g';
 *   ema != NULL: ema = ema_decay * ema + (1 - ema_decay) * p_new.
 * record: NULL, or the record m2t_grad_norm wrote on the same stream: clip_coef and the bias correction are read from it, and
 * with applied == 0 NOTHING is written (params, moments and ema keep every bit).  NULL: no clip, no skip, bias correction
 * from `step` on the host -- weight decay or EMA alone pay for no norm pass.  grads is never written: after the step it
 * still holds the raw gradient and the record holds the coefficient.  Buffers: device, 16-byte aligned.
 * M2T_ERR_ARG (decided on the host): n < 0, a null params / grads / moment buffer with n > 0, step < 1, weight_decay < 0,
 * ema_decay outside [0, 1). */
int m2t_adam_step_ex(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                     float beta1, float beta2, float eps, int step, float grad_scale, float* ema, float weight_decay,
                     int decoupled, float ema_decay, const double* record, void* stream);

/* ---- measurement: per-kernel-category timing with HIP events recorded on the launch stream.
 * category ids are listed in m2trans_amd/profile.py; mask bit i enables category i; 0 = off. */
int m2t_profile_enable(unsigned long long category_mask);
int m2t_profile_read(int category, double* total_ms, long long* launches);
/* single-kernel categories (attention, 3x3 conv, tail kernels) are timed by events that ride on the dispatch itself; such a
 * dispatch costs ~10 us of launch path, so a step with 16 timed launches runs 2 % slower than an untimed one.  n > 1 times a
 * uniform sample -- every n-th launch of each category -- instead (process-wide, default 1 = every launch); m2t_profile_read
 * then returns the total and the count of the SAMPLED launches. */
int m2t_profile_sample_every(int n);

/* ---- operators (NHWC tensors in `dtype` unless stated) ---------------------------------- */
/* DWT.forward / IWT.forward (models/M2Trans_network.py:198-237), `levels` in {1,2} applied
 * back-to-back; bit-exact in float32.  src [B,H,W,C] <-> dst [B,H/2^l,W/2^l,C*4^l]. */
int m2t_dwt(int dtype, int levels, const void* src, void* dst, int B, int H, int W, int C, void* stream);
int m2t_iwt(int dtype, int levels, const void* src, void* dst, int B, int H, int W, int C, void* stream);
/* nn.PixelShuffle(r) / its inverse on NCHW float32 (models/M2Trans_network.py:43,46,53): bit-exact.
 * in [B,C*r*r,H,W] -> out [B,C,H*r,W*r]. */
int m2t_pixel_shuffle(const float* in, float* out, int B, int C, int H, int W, int r, void* stream);
int m2t_pixel_unshuffle(const float* in, float* out, int B, int C, int H, int W, int r, void* stream);
/* NCHW float32 -> NHWC dtype and back. */
int m2t_to_nhwc(int dtype, const float* nchw, void* nhwc, int B, int C, int HW, void* stream);
int m2t_to_nchw(int dtype, const void* nhwc, float* nchw, int B, int C, int HW, void* stream);
/* TBlock.forward after the qkv projection (models/M2Trans_network.py:310-332):
 * qkv [B,h,w,3C] (q|k|v), rel_h/rel_w float32 [10*C/2] -> out [B,h,w,C]; C in {16,64,256}. */
int m2t_window_attention_fwd(int dtype, const void* qkv, const float* rel_h, const float* rel_w, void* out,
                             int B, int h, int w, int C, void* stream);
/* its autograd: gout [B,h,w,C] -> gqkv [B,h,w,3C], grel_h/grel_w float32 [10*C/2].
 * scratch: m2t_window_attention_bwd_scratch_bytes(dtype,B,h,w,C) bytes. */
size_t m2t_window_attention_bwd_scratch_bytes(int dtype, int B, int h, int w, int C);
int m2t_window_attention_bwd(int dtype, const void* qkv, const float* rel_h, const float* rel_w, const void* gout,
                             void* gqkv, float* grel_h, float* grel_w, void* scratch, int B, int h, int w, int C,
                             void* stream);

/* ---- SemanticLoss (losses.py:18-81): MedCLIP image tower = Swin-T 224 forward + the loss value ----
 * Forward only by default; opt-in gradient.  The reference evaluates it under torch.no_grad() (losses.py:63), so by
 * default it contributes a constant to the logged loss and no gradient.  The opt-in differentiable mode (SemanticLoss(...,
 * differentiable=True)) gives d total / d sr for total = sum_i |a_i - b_i| / N, a_i = <e(x_i), t^_i>, b_i the same for
 * the HR crop, e = normalise(P . mean_tokens(LN(Swin(.)))): sign(a_i - b_i) / N . J_e(x_i)^T t^_i (sign(0) = 0), taken back
 * through the last random crop (a paste) or, for N = 1, through the adjoint of the bicubic resize.  The tower is frozen:
 * data gradients only.  Weights: ONE flat float32 buffer in the order reported
 * by m2t_swin_param_name() (HF swin-tiny checkpoint names of transformers 4.24 + "projection_head.weight"
 * [512,768], the MedCLIP vision projection).  (include/m2t_swin.h: the encode and backward calls with every stage as an
 * extra output.) */
typedef struct m2t_swin m2t_swin;
int m2t_swin_create(m2t_swin** out, int max_images, int dtype);
void m2t_swin_destroy(m2t_swin* p);
/* "workspace_bytes", "num_params", "num_param_tensors", "max_images", "param:<name>", "numel:<name>"; "ws:<region>" /
 * "wsn:<region>": byte offset / element count of a workspace region (packed, fbias, crops, A0, X, Hn, QKV, AO, MH, emb);
 * "gws:<region>" / "gwsn:<region>": the same for the grad workspace in the layout of the last
 * m2t_swin_grad_workspace_bytes(p, n_grad), -1 before any (stash regions: e0, s<stage>b<block>.xin | .qkv | .xmid | .gder,
 * m0..m2, xf, hnf; scratch: gR, gF, gT, gC, gQ, gA, MD; everything before gR: transposed weights).  Unknown key: -1. */
long long m2t_swin_query(const m2t_swin* p, const char* key);
const char* m2t_swin_param_name(const m2t_swin* p, int index);
/* once per weight set: converts / fuses the frozen weights into the workspace */
int m2t_swin_load_weights(m2t_swin* p, const float* weights, void* workspace, void* stream);
/* medmodel.encode_image on n 224x224 crops (createNRandompatches, losses.py:29-40):
 * src [n_src,3,Hs,Ws] float32 NCHW on the device, crops_host int[n][3] = (source index, row0, col0)
 * -> emb [n,512] float32, unit L2 norm. */
int m2t_swin_encode(m2t_swin* p, const float* src, int n_src, int Hs, int Ws, const int* crops_host, int n,
                    float* emb, void* workspace, void* stream);
/* the same with the source images in two tensors (source index < n_a: src_a, else src_b[index - n_a]): the SR and HR
 * batches of one training step (train.py:203-205) are encoded together without a torch.cat of 2 x B x 3 x Hs x Ws floats */
int m2t_swin_encode_pair(m2t_swin* p, const float* src_a, int n_a, const float* src_b, int n_b, int Hs, int Ws,
                         const int* crops_host, int n, float* emb, void* workspace, void* stream);
/* losses.py:71-79 for a batch: emb [2B,512] (SR embeddings then HR embeddings), text [B,512] (any norm)
 * -> per_sample[B] = |sr.t - hr.t| / n_patches, total[1] = their sum. */
int m2t_semantic_loss(const float* emb, const float* text, int B, int n_patches, float* per_sample, float* total,
                      void* stream);
/* F.interpolate(mode='bicubic', align_corners=True) (losses.py:53-54): src [NC,Hin,Win] -> dst [NC,Hout,Wout]. */
int m2t_bicubic_resize(const float* src, float* dst, int NC, int Hin, int Win, int Hout, int Wout, void* stream);
/* opt-in gradient.  Grad workspace for n_grad crops: transposed weights of the data-gradient GEMMs, the activation stash of
 * n_grad crops (13.7 M elements of the compute type per crop) and the backward's scratch. */
long long m2t_swin_grad_workspace_bytes(m2t_swin* p, int n_grad);
/* m2t_swin_encode_pair that also stashes what the backward needs for crops [0, n_grad) (the SR crops come first).  fp32: emb
 * bit-identical to m2t_swin_encode_pair; bf16: the MLP of stages 1 / 2 runs unfused (it stores gelu'), within the bf16
 * tolerance of the forward.  grad_ws: at least m2t_swin_grad_workspace_bytes(p, n_grad) bytes. */
int m2t_swin_encode_grad(m2t_swin* p, const float* src_a, int n_a, const float* src_b, int n_b, int Hs, int Ws,
                         const int* crops_host, int n, int n_grad, float* emb, void* workspace, void* grad_ws, void* stream);
/* d total / d emb of the SR half: g_emb[B,512] = sign(a_i - b_i) / n_patches . t_i / |t_i| (emb, text as m2t_semantic_loss). */
int m2t_semantic_loss_backward(const float* emb, const float* text, int B, int n_patches, float* g_emb, void* stream);
/* vector-Jacobian product of encode_image for the n_grad crops of the last m2t_swin_encode_grad (same n_grad and grad_ws,
 * else M2T_ERR_STATE): g_emb [n_grad,512] -> g_crops [n_grad,3,224,224] float32 (overwritten).  The residual-stream gradient is
 * fp32 in both modes; in bf16 the GEMM operands are rounded to bf16. */
int m2t_swin_backward(m2t_swin* p, const float* g_emb, int n_grad, float* g_crops, void* workspace, void* grad_ws, void* stream);
/* the exact adjoint of m2t_bicubic_resize, a deterministic gather (no atomics): g_dst [NC,Hout,Wout] -> g_src [NC,Hin,Win]
 * (overwritten). */
int m2t_bicubic_resize_backward(const float* g_dst, float* g_src, int NC, int Hin, int Win, int Hout, int Wout, void* stream);

/* ---- SemanticLoss text tower (losses.py:22-25,64-65,74): medmodel.encode_text ---------------------------------
 * BERT-base forward (Bio_ClinicalBERT geometry: 12 layers x 768, 12 heads, 3072 intermediate, vocab 28 996, LayerNorm eps
 * 1e-12, erf GELU) -> mean over the tokens of hidden states 1, 2 and -1 -> Linear(768, 512, no bias) -> unit L2 norm, as the
 * un-vendored `medclip` package defines MedCLIPTextModel.forward / MedCLIPModel.encode_text (PARITY UNPINNED: package and
 * checkpoint absent from the reference tree).  Forward only (torch.no_grad() in the reference, losses.py:63).
 * Weights: ONE flat float32 buffer in the order of m2t_text_param_name(): HF BertModel checkpoint names of transformers
 * 4.24 without `pooler.*`, then "projection_head.weight" [512,768]. */
typedef struct m2t_text m2t_text;
int m2t_text_create(m2t_text** out, int max_seqs, int max_len /* <= 128 */, int dtype);
void m2t_text_destroy(m2t_text* p);
/* "workspace_bytes", "num_params", "num_param_tensors", "max_seqs", "max_len", "param:<name>", "numel:<name>",
 * "ws:<region>" (byte offset in the workspace) / "wsn:<region>" (element count at max_seqs x max_len) for the regions
 * packed, fbias, ids, mask, X, XM, Y, QKV, AO, MH (plan element type; ids, mask int32) and pooled (float32).  After an encode
 * the first n * len rows of X, XM, Y, QKV, AO, MH hold the LAST layer's output, attention-block LayerNorm, fc2 + residual sum,
 * q|k|v, attention output and GELU(fc1); rows beyond n * len are not written. */
long long m2t_text_query(const m2t_text* p, const char* key);
const char* m2t_text_param_name(const m2t_text* p, int index);
int m2t_text_load_weights(m2t_text* p, const float* weights, void* workspace, void* stream);
/* ids_host, mask_host: int[n][len] in HOST memory (tokenizer output; position ids are 0..len-1 and token types 0, BertModel's
 * defaults).  The reference passes outputs['token_type_ids'] in the input_ids slot (losses.py:65): a caller that wants the
 * reference's value passes those zeros here.  -> emb [n][512] float32 on the device, unit norm.
 * A key is attended iff its mask value is non-zero; a sequence with NO attended key gets uniform weights 1 / len over its len
 * keys (what the additive finfo.min mask of transformers gives).  An id outside [0, 28996) is M2T_ERR_ARG, before any launch
 * or copy.  (include/m2t_text.h: the same call with BertModel's hidden_states as a second output.) */
int m2t_text_encode(m2t_text* p, const int* ids_host, const int* mask_host, int n, int len, float* emb, void* workspace,
                    void* stream);

/* ---- util/rlutrans.py TransBlock (dead code in the reference: nothing imports it) --------------------
 * TransBlock.forward (util/rlutrans.py:82-87) for dim = 64, 8 heads: x + EffAttention(LayerNorm(x)) (:30-67: reduce,
 * qkv, softmax attention inside token chunks of length N // 16, proj), then x + Mlp(LayerNorm(x)) (:11-27: 64 -> 16,
 * ReLU, 16 -> 64).  Forward only.  params: the 22 928 float32 values of TransBlock(n_feat=64, dim=64).state_dict() in
 * state_dict order (atten.reduce.weight, atten.qkv.weight, atten.proj.weight, atten.proj.bias, norm1.weight,
 * norm1.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, norm2.weight, norm2.bias); x, y [B,N,64]
 * float32 on the device (y may alias x); dtype = compute element type (0 fp32, 1 bf16); N >= 16. */
size_t m2t_transblock_workspace_bytes(int B, int N, int dtype);
int m2t_transblock_forward(const float* params, const float* x, float* y, int B, int N, int dtype, void* workspace,
                           void* stream);

/* ---- evaluation metrics of the reference's test loop ------------------------------------------
 * test.py:101-113 / train.py:299-312: Y channel of utils.rgb_to_ycbcr (utils.py:121-146), `crop` (= scale) border
 * pixels removed, x255 when rgb_range == 1; then utils.calc_psnr (utils.py:179-184) and utils.calc_ssim
 * (utils.py:232-234 -> pytorch_msssim.ssim defaults).  sr, hr: float32 NCHW [B,3,H,W] on the device.
 * out: double[B][2] on the device = { mean(((Ysr-Yhr)/255)^2), mean SSIM } per image (PSNR = -10 log10 out[b][0]).
 * Y is bit-identical to the reference's fp32 Y; the reductions and the SSIM filtering are fp64.
 * window_host: the 11 fp32 taps of the SSIM window in HOST memory (the dependency computes them with torch.exp in
 * fp32, whose last bit a caller may want to reproduce), or NULL for the built-in exp(-(i-5)^2/4.5) normalised in fp32. */
size_t m2t_eval_metrics_scratch_bytes(int B, int H, int W, int crop);
int m2t_eval_metrics(const float* sr, const float* hr, int B, int H, int W, int crop, float rgb_range,
                     const float* window_host, void* scratch, double* out, void* stream);

/* piq.gmsd(hr, sr, data_range=1., reduction='none') of the same loop (test.py:98): gradient magnitude similarity deviation of
 * the 2x2-pooled luminance (0.299 R + 0.587 G + 0.114 B), Prewitt gradients, t = 170 / 255^2, population standard deviation of
 * the similarity map.  x, y: float32 NCHW [B,3,H,W] on the device; out: double[B] on the device.  The dependency (`piq`) is
 * absent from the reference tree: PARITY UNPINNED, checked against an fp64 restatement of the published algorithm. */
size_t m2t_eval_gmsd_scratch_bytes(int B);
int m2t_eval_gmsd(const float* x, const float* y, int B, int H, int W, float data_range, void* scratch, double* out, void* stream);

/* piq.fsim(hr, sr, data_range=1., reduction='none') of the same loop (test.py:95-96; piq 0.8.0 per environment.yml:118): FSIMc --
 * k x k average pooling (k = max(1, round(min(H, W) / 256))), YIQ, phase congruency from a 4-orientation x 4-scale log-Gabor bank
 * (explicit 2-D DFTs, any image size), Scharr gradient magnitude, chroma similarity, sum(S_L S_C^0.03 PC_m) / sum(PC_m).  fp64 on the
 * device (k_fsim.hip).  x, y: float32 NCHW [B,3,H,W] on the device; out: double[B] on the device; scratch:
 * m2t_eval_fsim_scratch_bytes(H, W) bytes (independent of B: image pairs are processed one after the other).
 * The dependency is absent from the reference tree: PARITY UNPINNED, checked against oracle/fsim_oracle.py. */
size_t m2t_eval_fsim_scratch_bytes(int H, int W);
int m2t_eval_fsim(const float* x, const float* y, int B, int H, int W, float data_range, void* scratch, double* out, void* stream);

/* ---- training input pipeline --------------------------------------------------------------------
 * datas/us1k.py:16-36 crop_patch + utils.py ndarray2tensor + the /255 of datas/us1k.py:169, for n samples at once,
 * cut out of uint8 HWC images that stay resident in device memory (lr_pool / hr_pool: the npy cache, back to back).
 * desc_host: long long[n][8] in HOST memory = { byte offset of the LR image in lr_pool, of the HR image in hr_pool,
 * LR row length in pixels, HR row length in pixels, lx, ly (LR corner; HR corner = scale x), flags (bit0 [:, ::-1],
 * bit1 [::-1, :], bit2 transpose(1,0,2), applied in that order like the reference), LR image height }.
 * lr_out [n,channels,patch/scale,patch/scale], hr_out [n,channels,patch,patch]: float32 NCHW, bit-identical to the
 * reference's tensors.  The random draws themselves stay with the caller (reference order: lx, ly, hflip, vflip, rot). */
int m2t_crop_patches(const unsigned char* lr_pool, const unsigned char* hr_pool, const long long* desc_host, int n,
                     int channels, int patch_size, int scale, float* lr_out, float* hr_out, void* stream);

/* datas/benchmark.py:62-72 (`Benchmark.__getitem__`): top-left h x w crop of a uint8 HWC image [img_h,img_w,channels]
 * resident in device memory -> float32 [channels,h,w] / 255, bit-identical to ndarray2tensor(...)/255. */
int m2t_image_to_tensor(const unsigned char* img, int img_h, int img_w, int channels, int h, int w, float* out, void* stream);
/* train.py:177-181: utils.cutmix (utils.py:16-71) and utils.cut_out (utils.py:74-108) on a device batch.  The random
 * draws stay with the caller (m2trans_amd/augment.py mirrors the reference's order); table_dev: int[B][1 + 5 * max_boxes]
 * on the device = { n, then n x (x1, y1, x2, y2, source sample) } in the order the reference applies the boxes.
 * mode 0 = cutmix: a pixel takes the value of the LAST covering box's source sample in the ORIGINAL tensor;
 * mode 1 = cut_out: a covered pixel is multiplied by 0.  mult scales the boxes (1 for LR, `scale` for HR, utils.py:49).
 * src, dst: float32 [B,C,H,W], distinct buffers.  Bit-identical to the reference's tensors. */
int m2t_box_mix(const float* src, float* dst, int B, int C, int H, int W, const int* table_dev, int max_boxes, int mode,
                int mult, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
