"""CPU yardstick of the optimizer pass with options (m2t_grad_norm + m2t_adam_step_ex, m2trans_amd/csrc/k_optim.hip): numpy only.

``step_f32`` restates the kernel's fp32 ROUNDING POINTS -- one IEEE operation per numpy operation, in the kernel's order (the
library is built with -ffp-contract=off, its division and square root are correctly rounded) -- and ``step_f64`` evaluates the
same step in fp64 from the same fp32 inputs.  The hyper-parameters cross the C ABI as fp32, so both take them rounded to fp32
first (``hyper32``); a torch arm that should agree must be given those values (1 - float32(0.999) is 1.3e-5 away from 0.001).

    g' = (g grad_scale) coef ; coupled: g' = g' + wd p ; decoupled: p = p float32(1 - lr wd)
    m = b1 m + (1-b1) g' ; v = b2 v + ((1-b2) g') g' ; p = p - (lr/bc1) (m / (sqrt(v)/sqrt(bc2) + eps))
    ema = d ema + (1-d) p

Units of the gates (``deviations``): one fp32 rounding, 2^-24, of the sum of the magnitudes of the terms of m, v and ema --
U_m = 2^-24 (|b1 m| + (1-b1) G), U_v = 2^-24 (b2 v + (1-b2) G^2), U_e = 2^-24 (|d ema| + |(1-d) p|) -- and ulp(p) for p.  G is
the magnitude of the terms of g': |g c| without coupled decay, |g c| + wd |p| with it (g' itself may be far smaller there).
Coupled decay can cancel (g c + wd p near 0): ``cancelled`` marks the elements with |g'| < 2^-10 (|g c| + wd |p|), where the
step is ill-conditioned for ANY fp32 implementation; the p gates leave them out and cap their share."""
from __future__ import annotations

import math

import numpy as np

F = np.float32
EPS24 = 2.0 ** -24
CANCEL = 2.0 ** -10          # |g'| below this share of |g c| + wd |p| counts as cancelled
CANCEL_CAP = 1e-3            # at most this share of the elements may be left out of a p gate


def hyper32(**kw) -> dict:
    """The values the kernel sees: every hyper-parameter rounded to fp32, returned as Python floats."""
    return {k: (None if v is None else float(F(v))) for k, v in kw.items()}


def bias_terms(b1: float, b2: float, t: int):
    """(1 - b1^t, sqrt(1 - b2^t)) in fp64 from the fp32 betas: what the norm's second stage writes into the record."""
    b1, b2 = float(F(b1)), float(F(b2))
    return 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)


def norm64(g: np.ndarray, grad_scale: float = 1.0) -> float:
    """sqrt(sum (fp32(g grad_scale))^2) in fp64 on the fp32 data."""
    x = (np.asarray(g, dtype=F) * F(grad_scale)).astype(np.float64)
    return float(np.sqrt(np.dot(x, x)))


def clip_coef(norm: float, max_norm) -> float:
    """torch.nn.utils.clip_grad_norm_'s coefficient, in fp32: min(1, max_norm / (float(norm) + 1e-6)); 1 when off."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    with np.errstate(all="ignore"):
        c = F(max_norm) / (F(norm) + F(1e-6))
    return float(F(1.0) if c > F(1.0) else c)


def ulp32(x: np.ndarray) -> np.ndarray:
    """Spacing of fp32 at |x| (fp64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=F))).astype(np.float64)


def step_f32(p, g, m, v, ema=None, *, lr, b1, b2, eps, t, coef=1.0, wd=0.0, decoupled=False, ema_decay=None, grad_scale=1.0):
    """One step at the kernel's rounding points.  Returns (p, m, v, ema) as new fp32 arrays (ema None when not given)."""
    p, g, m, v = (np.array(a, dtype=F, copy=True) for a in (p, g, m, v))
    lr, b1, b2, eps, coef, wd, gs = F(lr), F(b1), F(b2), F(eps), F(coef), F(wd), F(grad_scale)
    bc1, bc2s = bias_terms(b1, b2, t)
    bc1, bc2s = F(bc1), F(bc2s)
    one = F(1.0)
    gi = g * gs * coef
    if wd != 0 and not decoupled:
        gi = gi + wd * p
    if wd != 0 and decoupled:
        p = p * F(1.0 - float(lr) * float(wd))
    m = b1 * m + (one - b1) * gi
    v = b2 * v + (one - b2) * gi * gi
    denom = np.sqrt(v) / bc2s + eps
    p = p - (lr / bc1) * (m / denom)
    if ema is not None:
        d = F(ema_decay)
        ema = d * np.array(ema, dtype=F, copy=True) + (one - d) * p
    assert all(a.dtype == F for a in (p, m, v)) and (ema is None or ema.dtype == F)
    return p, m, v, ema


def step_f64(p, g, m, v, ema=None, *, lr, b1, b2, eps, t, coef=1.0, wd=0.0, decoupled=False, ema_decay=None, grad_scale=1.0):
    """The same step in fp64 from the same fp32 inputs and fp32 hyper-parameters.  Returns a dict: p, m, v, ema, the decayed
    gradient gp, the update u = p_decayed - p_new, and the magnitudes the gate units are made of."""
    p, g, m, v = (np.asarray(a, dtype=F).astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, coef, wd, gs = (float(F(x)) for x in (lr, b1, b2, eps, coef, wd, grad_scale))
    bc1, bc2s = bias_terms(b1, b2, t)
    gc = g * gs * coef
    gp = gc.copy()
    coupled = wd != 0 and not decoupled
    if coupled:
        gp = gp + wd * p
    if wd != 0 and decoupled:
        p = p * (1.0 - lr * wd)
    g_mag = np.abs(gc) + wd * np.abs(p) if coupled else np.abs(gp)
    s_m = np.abs(b1 * m) + (1.0 - b1) * g_mag
    s_v = b2 * v + (1.0 - b2) * g_mag * g_mag
    m = b1 * m + (1.0 - b1) * gp
    v = b2 * v + (1.0 - b2) * gp * gp
    denom = np.sqrt(v) / bc2s + eps
    u = (lr / bc1) * (m / denom)
    out = {"p": p - u, "m": m, "v": v, "u": u, "gp": gp, "denom": denom, "s_m": s_m, "s_v": s_v, "ema": None,
           "g_mag": g_mag, "lr_over_bc1": lr / bc1}
    if ema is not None:
        d = float(F(ema_decay))
        e = np.asarray(ema, dtype=F).astype(np.float64)
        out["s_e"] = np.abs(d * e) + np.abs((1.0 - d) * out["p"])
        out["ema"] = d * e + (1.0 - d) * out["p"]
    return out


def cancelled(r64: dict) -> np.ndarray:
    """Elements where coupled decay cancels: |g'| < 2^-10 (|g c| + wd |p|)."""
    return np.abs(r64["gp"]) < CANCEL * r64["g_mag"]


def deviations(got, r64: dict) -> dict:
    """How far fp32 results (p, m, v, ema) sit from the fp64 evaluation: p as |dp| (absolute) and |dp| beyond 2 ulp(p), m / v /
    ema in their units.  Per-element fp64 arrays; cancelled elements are NOT removed here."""
    p, m, v, ema = got
    tiny = 2.0 ** -149          # one subnormal spacing: an underflowing operation counts as one rounding
    dp = np.abs(np.asarray(p, dtype=np.float64) - r64["p"])
    out = {"p_abs": dp, "p_beyond": np.maximum(0.0, dp - 2.0 * ulp32(r64["p"])),
           "m": np.abs(np.asarray(m, dtype=np.float64) - r64["m"]) / (EPS24 * r64["s_m"] + tiny),
           "v": np.abs(np.asarray(v, dtype=np.float64) - r64["v"]) / (EPS24 * r64["s_v"] + tiny)}
    if ema is not None:
        out["ema"] = np.abs(np.asarray(ema, dtype=np.float64) - r64["ema"]) / (EPS24 * r64["s_e"] + tiny)
    return out
