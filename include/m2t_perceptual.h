/* m2t_perceptual.h -- the VGG19 feature ("perceptual") loss of libm2t.so, value and gradient in HIP.
 *
 * A seventh header on the same library, under the conventions of m2t.h and m2t_vif.h (extern "C", raw device pointers, a hipStream_t
 * passed as void*, 0 / m2t_status / hipError_t as the result, m2t_last_error_string for the text); the six older headers are unchanged.
 * Every entry only launches: no allocation, no upload, no host synchronisation; they may sit inside a stream capture.
 *
 * What it replaces: PerceptualLoss of the reference's losses.py (:222-270), a weighted distance between VGG19 features of sr and hr.
 *
 * Definition.
 *   tower    VGG19's convolutions 1_1, 1_2, 2_1, 2_2, 3_1 .. 3_4, 4_1 .. 4_4, 5_1 (layers 0 .. 12 below; torchvision vgg19 names
 *            features.{0,2,5,7,10,12,14,16,19,21,23,25,28}.{weight,bias}), each 3 x 3 with zero padding 1 and followed by ReLU; a 2 x 2
 *            stride-2 max pool with floor sizes after blocks 1 to 4 (after layers 1, 3, 7, 11).
 *   taps     F_0 .. F_4 = relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 (the outputs of layers 0, 2, 4, 8, 12).
 *   input    (c(x) / R - mean) / std with the ImageNet mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225) of losses.py:235-236,
 *            R the data range, c the clamp to [0, R] when the clamp is on (x only; y is never clamped); one channel is repeated to
 *            three, and its gradient is the sum over the three.
 *   term     scale * sum_k w_k * mean(rho(F_k(x) - F_k(y))), rho one of the pixel-loss kinds of m2t.h (M2T_LOSS_L1 the default; smooth-L1
 *            and MSE are the reference's 'sl1' and 'l2'), the mean over all elements of tap k.
 *   gradient with respect to x only, through the clamp mask (the ends of the range pass) when the clamp is on.
 * Inference semantics: the reference names a VGG19_relu that it never defines; only a vgg19_bn wrapper that is never put in eval mode
 * exists there.  This library takes plain vgg19 weights; a vgg19_bn checkpoint is folded into weight and bias on the host in fp64
 * (m2trans_amd.losses.PerceptualLoss.load_vgg_state_dict).  Training-mode batch statistics are NOT reproduced.  No weights ship.
 *
 * Numerics.  bf16 compute only: dtype M2T_F32 is M2T_ERR_ARG (a later version may add it).  Weights are rounded to bf16 once at load;
 * activations are bf16 NHWC; convolutions accumulate in fp32 on the matrix cores (conv1_1, K = 27, on the vector unit with the fp32
 * normalised input), the fp32 bias is added before the ReLU, and each stored activation is rounded once.  The loss is computed from the
 * STORED (rounded) taps with fp64 partial sums folded in a fixed order; no atomics; two runs are bit-identical.  Backward: the gradient
 * between layers is bf16; the tap seed scale * w_k * rho'(F_x - F_y) / N_k is added in fp32 before that rounding; the ReLU mask is
 * `saved output > 0`; the pool gradient goes to the first maximum of the saved window in row-major order (as torch), and a row or
 * column that the floor dropped receives none; the data gradient of a convolution is the same implicit GEMM on flipped, transposed
 * weights packed at load; the last 64 -> 3 gradient is fp32, scaled by 1 / (std R) and ADDED into the caller's buffer.  The y half keeps
 * only its five taps, the x half every post-ReLU activation; masks and arg-maxes are recomputed from those.
 *
 * Sizes: min(H, W) >= 16 (relu5_1 is then 1 x 1); anything smaller is M2T_ERR_ARG before any launch.  B <= 32767. */
#ifndef M2T_PERCEPTUAL_H
#define M2T_PERCEPTUAL_H
#include "m2t.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct m2t_vgg m2t_vgg;

/* The tower object (host memory only).  dtype must be M2T_BF16. */
int m2t_vgg_create(m2t_vgg** out, int dtype);
void m2t_vgg_destroy(m2t_vgg* v);
/* "num_params" (floats of the flat weight vector), "num_param_tensors" (26), "param:<name>" / "numel:<name>" (offset / count in floats,
 * torchvision vgg19 names), "packed_bytes" (the device buffer m2t_vgg_load_weights fills), "loaded" (0 / 1); -1 for an unknown key. */
long long m2t_vgg_query(const m2t_vgg* v, const char* key);
const char* m2t_vgg_param_name(const m2t_vgg* v, int i);
/* weights: the flat fp32 vector on the device, in the order of m2t_vgg_param_name.  packed: "packed_bytes" bytes on the device that the
 * caller keeps alive while the tower is used; the kernels read only this buffer afterwards. */
int m2t_vgg_load_weights(m2t_vgg* v, const float* weights, void* packed, void* stream);

/* Bytes of device workspace of one loss call on [B, C, H, W] (C does not matter); more with want_grad != 0.  0 for an unsupported shape.
 * No initialisation needed. */
size_t m2t_vgg_workspace_bytes(int B, int H, int W, int want_grad);
/* Where a region starts (bytes; the same with and without want_grad), for audits and tests; (size_t)-1 for an unsupported shape, region or index.  All bf16 NHWC but region 2.
 *   region 0: the saved post-ReLU output of layer `index` (0 .. 12) of the x half, [B][H_l][W_l][C_l]
 *   region 1: tap `index` (0 .. 4) of the y half
 *   region 2: the partial sums of tap `index`, up to 256 doubles
 *   region 3: the gradient at the convolution output of layer `index` (0 .. 12), after that layer's ReLU mask (want_grad only)
 * H_l = H >> (number of pools before layer l), likewise W_l; C_l = 64, 64, 128, 128, 256 x 4, 512 x 5. */
size_t m2t_vgg_workspace_offset(int B, int H, int W, int region, int index);

/* The plan-free loss (behind losses.PerceptualLoss).  x [B,C,H,W] float32 on the device with image stride x_image_stride, channel stride
 * x_image_stride / C and row stride x_row_stride (elements); y contiguous [B,C,H,W]; C is 1 or 3.  kind / param: M2T_LOSS_* of m2t.h.
 *   loss_out[0] = (accumulate ? loss_out[0] : 0) + (float)(scale * sum_k tap_weights[k] * mean_k)
 *   per_tap_out[k] = mean_k                                  double[5] on the device, or NULL
 *   gx_add[q] += d term / dx[q]                              x's strides; where clamp != 0 and x[q] is outside [0, data_range] the element
 *                                                            is left alone; NULL = value only (no gradient launches)
 * workspace: m2t_vgg_workspace_bytes(B, H, W, gx_add != NULL) bytes.  M2T_ERR_STATE: no weights loaded.  M2T_ERR_ARG: a null argument,
 * B outside 1 .. 32767, C other than 1 or 3, min(H, W) < 16, a bad data_range / kind / param, tap weights or scale not finite, strides
 * that do not hold the image. */
int m2t_vgg_loss_tensor(const m2t_vgg* v, const float* x, const float* y, int B, int C, int H, int W, long long x_image_stride,
                        int x_row_stride, float data_range, int clamp, int kind, float param, const double* tap_weights, double scale,
                        float* gx_add, float* loss_out, double* per_tap_out, int accumulate, void* workspace, void* stream);

/* The same routine on the forward's pre-clamp output of a plan (rgb_range = R, the clamp on), adding into the seed that the immediate
 * pixel loss or the output-gradient setter of m2t.h materialised; exactly 0 in the reflect padding.  scale = weight, and tap k's mean
 * divides by divisor * C_k H_k W_k, divisor = the GLOBAL number of images (world * accum * B), so that rank shards and micro-batches
 * sum to the global mean.  vgg_workspace: m2t_vgg_workspace_bytes(B, Hs, Ws, 1).  State rules of m2t_ssim_loss: M2T_ERR_STATE without a
 * forward with saved activations, without a seed, after a deferred pixel loss, or without loaded weights. */
int m2t_vgg_loss(m2t_plan* p, const m2t_vgg* v, const float* hr, float weight, double divisor, float rgb_range, int kind, float param,
                 const double* tap_weights, float* loss_out, int accumulate, void* vgg_workspace, void* workspace, void* stream);

/* Operator entries (tests and audits).  bf16 NHWC device tensors.
 * m2t_vgg_conv_forward: layer 1 .. 12: out = relu(conv(in) + bias) [N,H,W,Cout_l]; layer 0: `in` is float32 [N,3,H,W] contiguous and
 *   goes through (t / data_range - mean) / std first (no clamp).
 * m2t_vgg_conv_backward: layer 1 .. 12: gin [N,H,W,Cin_l] = the data gradient of gout [N,H,W,Cout_l], times [relu_of > 0] when relu_of
 *   (bf16 [N,H,W,Cin_l]) is not NULL; layer 0: gin is float32 [N,3,H,W] and receives += the gradient / (std * data_range).
 * m2t_vgg_pool_forward: [N,H,W,C] -> [N,H/2,W/2,C].  m2t_vgg_pool_backward: a = the pool's saved input; gin [N,H,W,C]; relu != 0
 *   multiplies by [a > 0].  C a multiple of 8; H, W >= 2. */
int m2t_vgg_conv_forward(const m2t_vgg* v, int layer, const void* in, void* out, int N, int H, int W, float data_range, void* stream);
int m2t_vgg_conv_backward(const m2t_vgg* v, int layer, const void* gout, const void* relu_of, void* gin, int N, int H, int W,
                          float data_range, void* stream);
int m2t_vgg_pool_forward(const void* in, void* out, int N, int H, int W, int C, void* stream);
int m2t_vgg_pool_backward(const void* a, const void* gout, void* gin, int N, int H, int W, int C, int relu, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
