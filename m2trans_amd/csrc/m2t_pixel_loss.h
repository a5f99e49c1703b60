// The pixel-loss family of the training step: one per-pixel function for every kernel that takes the loss.
//
//   l1           |d|                                   models' criterion "l1"  (reference losses.py:225-230, train.py:76,199)
//   mse  (l2)    d^2                                   nn.MSELoss              (losses.py:225-230, "l2")
//   charbonnier  sqrt(d^2 + eps)                       L1_Charbonnier_loss     (losses.py:287-297; eps under the root, :295)
//   smooth_l1    |d| < beta ? d^2 / (2 beta)           nn.SmoothL1Loss         (losses.py:225-230, "sl1")
//     (sl1)               : |d| - beta / 2
//
// with d = clamp(pre, 0, R) - hr.  The callers -- clamp_l1_kernel / clamp_l1_vec4_kernel (k_pointwise.hip) and the two recomputing x4
// tail backward kernels (k_tail_bwd.hip) -- form
//
//   loss  = loss_scale * sum rho(d)                      loss_scale = sc = (float)(weight / divisor)
//   seed  = rho'(d)-factor * gscale * [0 <= pre <= R]    inside the crop, 0 elsewhere (the clamp mask inclusive, as torch.clamp's)
//
// where gscale = sc, except for mse: the 2 of (d^2)' is folded into gscale ONCE on the host (2 sc: exact in fp32), so that the factor is d
// itself.  All arithmetic in fp32; `kind` is wave-uniform -- every caller passes a template constant, the switch folds at compile time and
// the l1 instantiation is the code (and gives the bits) it was before the other kinds existed.
#pragma once
#include <cmath>

enum M2TPixelLossKind : int { M2T_PL_L1 = 0, M2T_PL_MSE = 1, M2T_PL_CHARBONNIER = 2, M2T_PL_SMOOTH_L1 = 3, M2T_PL_KINDS = 4 };

// what the host precomputes for one loss request (m2t_pixel_loss_make): the kernels receive these by value
struct M2TPixelLoss {
  int kind = M2T_PL_L1;
  float param = 0.f;        // charbonnier: eps; smooth_l1: beta; else unused
  float f0 = 0.f;           // smooth_l1: 1 / beta
  float f1 = 0.f;           // smooth_l1: beta / 2
  float loss_scale = 0.f;   // sc
  float gscale = 0.f;       // sc (mse: 2 sc)
};

// false: unknown kind, or a parameter that is not finite and > 0 where the kind needs one
inline bool m2t_pixel_loss_make(int kind, float param, float sc, M2TPixelLoss* out) {
  if (kind < 0 || kind >= M2T_PL_KINDS) return false;
  const bool needs = kind == M2T_PL_CHARBONNIER || kind == M2T_PL_SMOOTH_L1;
  if (needs && !(std::isfinite(param) && param > 0.f)) return false;
  M2TPixelLoss l;
  l.kind = kind;
  l.param = needs ? param : 0.f;
  if (kind == M2T_PL_SMOOTH_L1) { l.f0 = (float)(1.0 / (double)param); l.f1 = (float)(0.5 * (double)param); }
  l.loss_scale = sc;
  l.gscale = kind == M2T_PL_MSE ? 2.f * sc : sc;
  *out = l;
  return true;
}

#if defined(__HIPCC__)
// returns the seed factor, term = rho(d)
__device__ __forceinline__ float m2t_pixel_loss_eval(int kind, float d, float param, float f0, float f1, float& term) {
  if (kind == M2T_PL_MSE) {
    term = d * d;
    return d;
  }
  if (kind == M2T_PL_CHARBONNIER) {
    const float r = sqrtf(d * d + param);
    term = r;
    return d / r;
  }
  const float ad = fabsf(d);
  const float sg = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
  if (kind == M2T_PL_SMOOTH_L1) {
    const bool quad = ad < param;
    term = quad ? (0.5f * f0) * (d * d) : ad - f1;
    return quad ? d * f0 : sg;
  }
  term = ad;                // M2T_PL_L1
  return sg;
}
#endif
