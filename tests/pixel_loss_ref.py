"""fp64 restatement of TrainStep's pixel-loss family (include/m2t.h: m2t_pixel_loss): per-pixel term, derivative and the
clamp / crop mask of the backward seed.  With d = clamp(pre, 0, R) - hr:

    l1           |d|                                              sign(d), 0 at d = 0
    mse          d^2                                              2 d
    charbonnier  sqrt(d^2 + eps)                                  d / sqrt(d^2 + eps)
    smooth_l1    |d| < beta ? d^2 / (2 beta) : |d| - beta / 2     |d| < beta ? d / beta : sign(d)

    loss = (weight / divisor) * sum term(d)
    seed = (weight / divisor) * derivative(d) * [0 <= pre <= R]   inside the image, 0 in the padding

tests/test_pixel_loss_cpu.py pins this file to torch's own loss modules and autograd; the GPU tests compare the kernels with it.
"""
from __future__ import annotations

import torch

KINDS = {"l1": 0, "mse": 1, "charbonnier": 2, "smooth_l1": 3}
DEFAULT_PARAM = {"l1": None, "mse": None, "charbonnier": 1e-6, "smooth_l1": 1.0}


def _param(kind: str, param):
    return DEFAULT_PARAM[kind] if param is None else param


def term(kind: str, d: torch.Tensor, param=None) -> torch.Tensor:
    d = d.double()
    p = _param(kind, param)
    if kind == "l1":
        return d.abs()
    if kind == "mse":
        return d * d
    if kind == "charbonnier":
        return torch.sqrt(d * d + p)
    if kind == "smooth_l1":
        return torch.where(d.abs() < p, 0.5 * d * d / p, d.abs() - 0.5 * p)
    raise KeyError(kind)


def derivative(kind: str, d: torch.Tensor, param=None) -> torch.Tensor:
    d = d.double()
    p = _param(kind, param)
    if kind == "l1":
        return torch.sign(d)
    if kind == "mse":
        return 2.0 * d
    if kind == "charbonnier":
        return d / torch.sqrt(d * d + p)
    if kind == "smooth_l1":
        return torch.where(d.abs() < p, d / p, torch.sign(d))
    raise KeyError(kind)


def clamp_mask(pre: torch.Tensor, R: float = 1.0) -> torch.Tensor:
    """Where the clamp passes a gradient: inclusive at both ends, as torch.clamp's backward."""
    return (pre >= 0) & (pre <= R)


def loss_and_seed(kind: str, pre: torch.Tensor, hr: torch.Tensor, param=None, weight: float = 1.0, divisor=None, R: float = 1.0):
    """pre [B,3,Hp,Wp]: the pre-clamp output at the padded size; hr [B,3,Hs,Ws] with Hs <= Hp, Ws <= Wp (the image is the top-left
    corner).  Returns (loss: 0-d fp64, seed [B,3,Hp,Wp] fp64: 0 in the padding).  divisor defaults to hr.numel() (the mean)."""
    pre, hr = pre.double(), hr.double()
    Hs, Ws = hr.shape[-2:]
    sc = float(weight) / float(hr.numel() if divisor is None else divisor)
    inner = pre[..., :Hs, :Ws]
    d = inner.clamp(0.0, R) - hr
    loss = sc * term(kind, d, param).sum()
    seed = torch.zeros_like(pre)
    seed[..., :Hs, :Ws] = sc * derivative(kind, d, param) * clamp_mask(inner, R)
    return loss, seed
