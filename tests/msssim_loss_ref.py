"""fp64 restatement of the MS-SSIM loss term (include/m2t_msssim.h: m2t_msssim_loss_tensor / m2t_msssim_loss), per image b and
channel c, in the pytorch_msssim.ms_ssim / piq.multi_scale_ssim form, built on tests/ssim_loss_ref.py:

    x_0 = clamp(pre, 0, R) / R,  y_0 = hr / R                                  (data_range 1)
    five levels l = 0 .. 4, weights w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); window, constants, m1 .. B2 of ssim_loss_ref
    v_l = mean_map(A2 / B2) for l < 4 (contrast-structure),  v_4 = mean_map(A1 A2 / (B1 B2)) (SSIM)
    x_{l+1} = avg_pool2d(x_l, 2, 2, padding (H_l % 2, W_l % 2), zeros counted): every output is ((a + b) + c) + d) / 4 over its
              2 x 2 cell in row-major order, members outside the image counting as 0; an odd side starts its cells at index -1
    M_bc = prod_l max(v_l, 0)^{w_l};   loss = scale * sum_bc (1 - M_bc)

    gradient, all v_l > 0:  dM / dx_l = (w_l M / v_l) / n_l * d sum(map_l) / dx_l  (n_l map entries), with for the cs map
        dE = -cs / B2, dF = 2 / B2, dM = (-2 m2 + 2 m1 cs) / B2  (the SSIM expressions without A1 / B1);
        d / dx_0 = sum_l (P^T)^l d / dx_l, P^T the adjoint of the pooling (a fine pixel takes 1 / 4 of its one parent);
        seed = -scale / R * that * [0 <= pre <= R]
    any v_l <= 0:  M_bc = 0 and the gradient of that (b, c) is exactly 0 (torch's autograd gives 0 * inf there: not matched).

tests/test_msssim_loss_cpu.py pins the analytic gradient to torch autograd of `ms_ssim` and the pooling to F.avg_pool2d and to an
index loop; the GPU tests compare the kernels with this file.
"""
from __future__ import annotations

import torch

from tests import ssim_loss_ref as S

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
LEVELS = 5
MIN_SIDE = (S.WIN - 1) * 2 ** 4 + 1          # min(H, W) > 160


def pooled_side(n: int) -> int:
    return n // 2 + n % 2


def pool(t: torch.Tensor) -> torch.Tensor:
    """One level down: [..., H, W] -> [..., H/2 + H%2, W/2 + W%2], the members of a cell summed in row-major order."""
    H, W = t.shape[-2:]
    p = torch.zeros(t.shape[:-2] + (H + 2 * (H % 2), W + 2 * (W % 2)), dtype=t.dtype, device=t.device)
    p[..., H % 2:H % 2 + H, W % 2:W % 2 + W] = t
    Ho, Wo = pooled_side(H), pooled_side(W)
    p = p[..., :2 * Ho, :2 * Wo]
    return (((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + p[..., 1::2, 0::2]) + p[..., 1::2, 1::2]) * 0.25


def pool_t(g: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The adjoint of pool for a fine level of H x W: every fine pixel takes 1 / 4 of its one parent."""
    iy = (torch.arange(H, device=g.device) + H % 2) // 2
    ix = (torch.arange(W, device=g.device) + W % 2) // 2
    return 0.25 * g[..., iy, :][..., :, ix]


def pyramid(t: torch.Tensor):
    """[t, pool(t), ..., pool^4(t)]."""
    out = [t]
    for _ in range(LEVELS - 1):
        out.append(pool(out[-1]))
    return out


def cs_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    _, _, _, _, A2, _, B2 = S._parts(x, y)
    return A2 / B2


def level_values(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """v [B, C, 5] of images already scaled to data_range 1, in the dtype of x."""
    xs, ys = pyramid(x), pyramid(y)
    v = [cs_map(xs[l], ys[l]).mean(dim=(-2, -1)) for l in range(LEVELS - 1)]
    v.append(S.ssim_map(xs[-1], ys[-1]).mean(dim=(-2, -1)))
    return torch.stack(v, dim=-1)


def ms_ssim(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """M [B, C]: prod_l max(v_l, 0)^{w_l}; exactly 0 where any v_l <= 0.  Differentiable by autograd where every v_l > 0 (with a
    non-positive v_l autograd forms 0 * inf: use value_and_grad)."""
    v = level_values(x, y)
    w = torch.tensor(WEIGHTS, dtype=v.dtype, device=v.device)
    return (v.clamp(min=0.0) ** w).prod(dim=-1)


def dcs_dx(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """d sum(cs) / dx, analytic."""
    g, m1, m2, _, A2, _, B2 = S._parts(x, y)
    cs = A2 / B2
    dE = -cs / B2
    dF = 2.0 / B2
    dM = (-2.0 * m2 + 2.0 * m1 * cs) / B2
    return S._filt_t(dM, g) + 2 * x * S._filt_t(dE, g) + y * S._filt_t(dF, g)


def value_and_grad(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, clamp: bool = False, scale: float = 1.0):
    """The plan-free entry for raw x, y [B,C,H,W], fp64: (scale * sum_bc (1 - M_bc), the gradient of that with respect to x
    [through the clamp mask], M [B,C], the level gradients G_1 .. G_4 = dM_bc / dx_l)."""
    x, y = x.double(), y.double()
    xn = (x.clamp(0.0, data_range) if clamp else x) / data_range
    yn = y / data_range
    xs, ys = pyramid(xn), pyramid(yn)
    v = level_values(xn, yn)
    alive = (v > 0).all(dim=-1)                                            # [B, C]
    w = torch.tensor(WEIGHTS, dtype=torch.float64)
    M = torch.where(alive, (v.clamp(min=0.0) ** w).prod(dim=-1), torch.zeros_like(alive, dtype=torch.float64))
    G, levels = None, []
    for l in range(LEVELS - 1, -1, -1):
        n_l = (xs[l].shape[-2] - S.WIN + 1) * (xs[l].shape[-1] - S.WIN + 1)
        coef = torch.where(alive, w[l] * M / (v[..., l] * n_l), torch.zeros_like(M))
        d = S.dsum_dx(xs[l], ys[l]) if l == LEVELS - 1 else dcs_dx(xs[l], ys[l])
        own = coef[..., None, None] * d
        G = own if G is None else own + pool_t(G, *xs[l].shape[-2:])
        G = torch.where(alive[..., None, None], G, torch.zeros_like(G))
        levels.append(G)
    value = scale * (1.0 - M).sum()
    grad = -scale / data_range * G
    if clamp:
        grad = grad * ((x >= 0) & (x <= data_range))
    return value, grad, M, levels[::-1][1:]


def loss_and_seed(pre: torch.Tensor, hr: torch.Tensor, weight: float = 1.0, divisor=None, R: float = 1.0):
    """pre [B,3,Hp,Wp]: the pre-clamp output at the padded size; hr [B,3,Hs,Ws] (the image is the top-left corner), the layout of
    ssim_loss_ref.loss_and_seed.  Returns (loss: 0-d fp64, seed [B,3,Hp,Wp] fp64: 0 in the padding).  divisor defaults to the number
    of (image, channel) pairs (the mean)."""
    pre, hr = pre.double(), hr.double()
    Hs, Ws = hr.shape[-2:]
    n = hr.shape[0] * hr.shape[1]
    sc = float(weight) / float(n if divisor is None else divisor)
    loss, g, _, _ = value_and_grad(pre[..., :Hs, :Ws], hr, R, True, sc)
    seed = torch.zeros_like(pre)
    seed[..., :Hs, :Ws] = g
    return loss, seed


def smooth_pair(shape, sigma: float, seed: int = 0, R: float = 1.0, spill: bool = False):
    """(x, y) float32 of the kind the gradient comparisons use: y = R * smoothed uniform noise, x = y + R * sigma * randn, clamped
    to [0, R] -- or, with `spill`, stretched about its 5 % and 95 % quantiles instead, so that a tenth of x lies outside [0, R]."""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    u = torch.rand(B, C, H + 8, W + 8, generator=g, dtype=torch.float64)
    k = torch.ones(1, 1, 9, 9, dtype=torch.float64) / 81.0
    y = torch.nn.functional.conv2d(u.view(B * C, 1, H + 8, W + 8), k).view(B, C, H, W)
    y = (y - y.min()) / (y.max() - y.min())
    x = y + sigma * torch.randn(shape, generator=g, dtype=torch.float64)
    if spill:
        lo, hi = torch.quantile(x.flatten(), 0.05), torch.quantile(x.flatten(), 0.95)
        x = (x - lo) / (hi - lo)
    else:
        x = x.clamp(0.0, 1.0)
    return (x * R).float().contiguous(), (y * R).float().contiguous()
