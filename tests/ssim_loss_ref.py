"""fp64 restatement of the SSIM loss term (include/m2t.h: m2t_ssim_loss_tensor / m2t_ssim_loss), per channel, in the
pytorch_msssim.ssim / piq.ssim(downsample=False) form:

    x = clamp(pre, 0, R) / R,  y = hr / R                              (data_range 1)
    G = separable 11-tap Gaussian, sigma 1.5, VALID; taps = the fp32-normalised window widened to fp64
    m1 = G*x, m2 = G*y, s1 = G*(x^2) - m1^2, s2 = G*(y^2) - m2^2, s12 = G*(xy) - m1 m2;  C1 = 1e-4, C2 = 9e-4
    A1 = 2 m1 m2 + C1, A2 = 2 s12 + C2, B1 = m1^2 + m2^2 + C1, B2 = s1 + s2 + C2;  S = A1 A2 / (B1 B2)   (no clamp of S)
    loss = (weight / divisor) * sum_map (1 - S)

    dE = -A1 A2 / (B1 B2^2), dF = 2 A1 / (B1 B2), dM = 2 m2 (A2 - A1) / (B1 B2) - 2 m1 S / B1 + 2 m1 S / B2
    d sum(S) / dx(q) = (G^T*dM)(q) + 2 x(q) (G^T*dE)(q) + y(q) (G^T*dF)(q)     G^T* = full correlation, zeros outside the map
    seed = -(weight / divisor) / R * that * [0 <= pre <= R]   inside the image, 0 in the padding

piq.SSIMLoss's default downsample=True (average pooling in front) is not part of it.  tests/test_ssim_loss_cpu.py pins the analytic
gradient to torch autograd and the value to an independent scipy evaluation; the GPU tests compare the kernels with this file.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import m2trans_oracle as O

C1, C2 = 0.01 ** 2, 0.03 ** 2
WIN = 11


def taps(dtype=torch.float64) -> torch.Tensor:
    return O.ssim_window(torch.float32).to(dtype)


def _filt(t: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """VALID separable correlation of [B,C,H,W], first along H then along W, one filter per channel."""
    c = t.shape[1]
    t = F.conv2d(t, g.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)
    return F.conv2d(t, g.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)


def _filt_t(t: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """The transpose of _filt: [B,C,H-10,W-10] -> [B,C,H,W]."""
    c = t.shape[1]
    t = F.conv_transpose2d(t, g.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)
    return F.conv_transpose2d(t, g.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)


def _parts(x: torch.Tensor, y: torch.Tensor):
    g = taps(x.dtype).to(x.device)
    m1, m2 = _filt(x, g), _filt(y, g)
    s1, s2, s12 = _filt(x * x, g) - m1 * m1, _filt(y * y, g) - m2 * m2, _filt(x * y, g) - m1 * m2
    return g, m1, m2, 2 * m1 * m2 + C1, 2 * s12 + C2, m1 * m1 + m2 * m2 + C1, s1 + s2 + C2


def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """S [B,C,H-10,W-10] of images already scaled to data_range 1, in the dtype of x (fp64 for the reference, fp32 for the
    'torch route' arm of the TrainStep test)."""
    _, _, _, A1, A2, B1, B2 = _parts(x, y)
    return A1 * A2 / (B1 * B2)


def dsum_dx(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """d sum(S) / dx, analytic."""
    g, m1, m2, A1, A2, B1, B2 = _parts(x, y)
    S = A1 * A2 / (B1 * B2)
    dE = -A1 * A2 / (B1 * B2 * B2)
    dF = 2 * A1 / (B1 * B2)
    dM = 2 * m2 * (A2 - A1) / (B1 * B2) - 2 * m1 * S / B1 + 2 * m1 * S / B2
    return _filt_t(dM, g) + 2 * x * _filt_t(dE, g) + y * _filt_t(dF, g)


def value_and_grad(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, clamp: bool = False, scale: float = 1.0):
    """The plan-free entry: (scale * sum(1 - S), -scale * d sum(S) / dx [through the clamp mask]) for raw x, y [B,C,H,W], fp64."""
    x, y = x.double(), y.double()
    xn = (x.clamp(0.0, data_range) if clamp else x) / data_range
    yn = y / data_range
    value = scale * (1.0 - ssim_map(xn, yn)).sum()
    grad = -scale / data_range * dsum_dx(xn, yn)
    if clamp:
        grad = grad * ((x >= 0) & (x <= data_range))
    return value, grad


def loss_and_seed(pre: torch.Tensor, hr: torch.Tensor, weight: float = 1.0, divisor=None, R: float = 1.0):
    """pre [B,3,Hp,Wp]: the pre-clamp output at the padded size; hr [B,3,Hs,Ws] (the image is the top-left corner), the layout of
    pixel_loss_ref.loss_and_seed.  Returns (loss: 0-d fp64, seed [B,3,Hp,Wp] fp64: 0 in the padding).  divisor defaults to the
    number of map entries (the mean)."""
    pre, hr = pre.double(), hr.double()
    Hs, Ws = hr.shape[-2:]
    n = hr.shape[0] * hr.shape[1] * (Hs - WIN + 1) * (Ws - WIN + 1)
    sc = float(weight) / float(n if divisor is None else divisor)
    loss, g = value_and_grad(pre[..., :Hs, :Ws], hr, R, True, sc)
    seed = torch.zeros_like(pre)
    seed[..., :Hs, :Ws] = g
    return loss, seed
