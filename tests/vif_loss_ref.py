"""fp64 restatement of the VIF loss term (include/m2t_vif.h: m2t_vif_loss_tensor / m2t_vif_loss), pixel domain, per image b:

    u_0 = (255 / R) * (0.299 c(x_R) + 0.587 c(x_G) + 0.114 c(x_B)), c = clamp to [0, R] when the clamp is on; v_0 of y, never clamped;
          one channel: u_0 = 255 / R * c(x)
    scales s = 0 .. 3, N_s = 2^(4 - s) + 1 taps g_s[k] = exp(-(k - (N_s - 1) / 2)^2 / (2 (N_s / 5)^2)) / sum, separable, VALID
    u_s = (G_s * u_{s-1})[::2, ::2] for s > 0, v_s likewise
    mx = G*u, my = G*v, a = max(G*(uu) - mx^2, 0), b = max(G*(vv) - my^2, 0), c = G*(uv) - mx my
    live = b >= EPS and a >= EPS and c >= 0;  g = c / (b + EPS);  sv_raw = a - g c;  sv = sv_raw if sv_raw > EPS else EPS
    t = log10(1 + g^2 b / (sv + n)) where live, 0 elsewhere;   d = log10(1 + b / n) where b >= EPS, 0 elsewhere
    VIF_b = (sum t + EPS) / (sum d + EPS);   loss = scale * sum_b (1 - VIF_b)

    gradient (x only), where live, q = g^2 b, z = sv + n, k = 1 / (ln 10 (1 + q / z)):
        dt/da = -k q / z^2 if sv_raw > EPS else 0
        dt/dc = k (2 c b / ((b + EPS)^2 z) + (q / z^2) (2 c / (b + EPS) if sv_raw > EPS else 0))
        d sum(t_s) / du_s = 2 u G^T[dt/da] + v G^T[dt/dc] + G^T[-2 mx dt/da - my dt/dc]
        G_s = that + the adjoint of (filter G_{s+1}, decimate) of G_{s+1};  dVIF_b / du_0 = G_0 / (sum d + EPS)
        to channel ch: times w_ch * 255 / R * [0 <= x_ch <= R] (the mask with the clamp on only)

tests/test_vif_loss_cpu.py pins the analytic gradient to torch autograd of `vif` and the pyramid to F.conv2d(...)[..., ::2, ::2]; the
GPU tests and the host emulation compare the kernels with this file.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

EPS = 1e-8
SCALES = 4
MIN_SIDE = 41
LUMA = (0.299, 0.587, 0.114)


def win_len(s: int) -> int:
    return 2 ** (4 - s) + 1


def taps(s: int) -> torch.Tensor:
    n = win_len(s)
    k = torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0
    g = torch.exp(-(k * k) / (2.0 * (n / 5.0) ** 2))
    return g / g.sum()


def luminance(t: torch.Tensor, R: float, clamp: bool) -> torch.Tensor:
    """[B,C,H,W] (C = 1 or 3) -> [B,H,W] fp64 on the 0 .. 255 scale."""
    t = t.double()
    if clamp:
        t = t.clamp(0.0, R)
    k = 255.0 / R
    if t.shape[1] == 3:
        return k * (LUMA[0] * t[:, 0] + LUMA[1] * t[:, 1] + LUMA[2] * t[:, 2])
    assert t.shape[1] == 1, "VIF takes 1 or 3 channels"
    return k * t[:, 0]


def filt(t: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """[B,H,W] under the separable window g, VALID."""
    n = g.numel()
    t = F.conv2d(t[:, None], g.view(1, 1, n, 1))
    return F.conv2d(t, g.view(1, 1, 1, n))[:, 0]


def filt_t(m: torch.Tensor, g: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """The adjoint of filt (stride 1), or of filt followed by [::stride, ::stride]."""
    n = g.numel()
    m = F.conv_transpose2d(m[:, None], g.view(1, 1, 1, n), stride=(1, stride))
    return F.conv_transpose2d(m, g.view(1, 1, n, 1), stride=(stride, 1))[:, 0]


def down(t: torch.Tensor, s: int) -> torch.Tensor:
    """Level s from level s - 1."""
    return filt(t, taps(s))[:, ::2, ::2]


def down_t(gr: torch.Tensor, s: int, H: int, W: int) -> torch.Tensor:
    """The adjoint of down(., s) for a finer level of H x W: zero-stuffing by 2, the transposed G_s, zeros beyond."""
    out = filt_t(gr, taps(s), stride=2)
    return F.pad(out, (0, W - out.shape[-1], 0, H - out.shape[-2]))


def pyramid(t: torch.Tensor):
    out = [t]
    for s in range(1, SCALES):
        out.append(down(out[-1], s))
    return out


def moments(u, v, s):
    g = taps(s)
    mx, my = filt(u, g), filt(v, g)
    a = (filt(u * u, g) - mx * mx).clamp(min=0.0)
    b = (filt(v * v, g) - my * my).clamp(min=0.0)
    c = filt(u * v, g) - mx * my
    return g, mx, my, a, b, c


def _maps(a, b, c, n):
    live = (b >= EPS) & (a >= EPS) & (c >= 0)
    gg = c / (b + EPS)
    sv_raw = a - gg * c
    is_open = sv_raw > EPS
    sv = torch.where(is_open, sv_raw, torch.full_like(sv_raw, EPS))
    q = gg * gg * b
    z = sv + n
    t = torch.where(live, torch.log10(1.0 + q / z), torch.zeros_like(q))
    d = torch.where(b >= EPS, torch.log10(1.0 + b / n), torch.zeros_like(b))
    return live, is_open, q, z, t, d


def vif(u0: torch.Tensor, v0: torch.Tensor, sigma_n_sq: float = 2.0) -> torch.Tensor:
    """VIF [B] of two luminance planes [B,H,W]; differentiable by autograd."""
    us, vs = pyramid(u0), pyramid(v0)
    num = torch.zeros(u0.shape[0], dtype=u0.dtype)
    den = torch.zeros(u0.shape[0], dtype=u0.dtype)
    for s in range(SCALES):
        _, _, _, a, b, c = moments(us[s], vs[s], s)
        _, _, _, _, t, d = _maps(a, b, c, sigma_n_sq)
        num = num + t.sum(dim=(-2, -1))
        den = den + d.sum(dim=(-2, -1))
    return (num + EPS) / (den + EPS)


def details(x, y, R=1.0, clamp=False, sigma_n_sq=2.0):
    """(VIF [B], sum d [B], the u pyramid, the v pyramid, the level gradients G_0 .. G_3 = d sum(t) / du_s, the branch shares)."""
    u0, v0 = luminance(x, R, clamp), luminance(y, R, False)
    us, vs = pyramid(u0), pyramid(v0)
    num = torch.zeros(u0.shape[0], dtype=torch.float64)
    den = torch.zeros(u0.shape[0], dtype=torch.float64)
    own, shares = [], []
    for s in range(SCALES):
        g, mx, my, a, b, c = moments(us[s], vs[s], s)
        live, is_open, q, z, t, d = _maps(a, b, c, sigma_n_sq)
        num = num + t.sum(dim=(-2, -1))
        den = den + d.sum(dim=(-2, -1))
        k = 1.0 / (math.log(10.0) * (1.0 + q / z))
        zero = torch.zeros_like(q)
        be = b + EPS
        dA = torch.where(live & is_open, -k * q / (z * z), zero)
        dC = torch.where(live, k * (2.0 * c * b / (be * be * z) + (q / (z * z)) * torch.where(is_open, 2.0 * c / be, zero)), zero)
        dU = -2.0 * mx * dA - my * dC
        own.append(2.0 * us[s] * filt_t(dA, g) + vs[s] * filt_t(dC, g) + filt_t(dU, g))
        n = float(live.numel())
        shares.append({"dead": float((~live).sum()) / n, "clamped": float((live & ~is_open).sum()) / n, "live": float((live & is_open).sum()) / n})
    G = [None] * SCALES
    for s in range(SCALES - 1, -1, -1):
        G[s] = own[s] if s == SCALES - 1 else own[s] + down_t(G[s + 1], s + 1, *us[s].shape[-2:])
    return (num + EPS) / (den + EPS), den, us, vs, G, shares


def value_and_grad(x, y, R: float = 1.0, clamp: bool = False, scale: float = 1.0, sigma_n_sq: float = 2.0):
    """The plan-free entry for raw x, y [B,C,H,W], fp64: (scale * sum_b (1 - VIF_b), the gradient of that with respect to x [through
    the clamp mask], VIF [B], per-scale branch shares [{dead, clamped, live}])."""
    x = x.double()
    v, den, _, _, G, shares = details(x, y, R, clamp, sigma_n_sq)
    du0 = G[0] / (den + EPS)[:, None, None]
    C = x.shape[1]
    w = torch.tensor(LUMA if C == 3 else (1.0,), dtype=torch.float64)
    grad = -scale * (255.0 / R) * w[None, :, None, None] * du0[:, None]
    if clamp:
        grad = grad * ((x >= 0) & (x <= R))
    return scale * (1.0 - v).sum(), grad, v, shares


def loss_and_seed(pre, hr, weight: float = 1.0, divisor=None, R: float = 1.0, sigma_n_sq: float = 2.0):
    """pre [B,3,Hp,Wp]: the pre-clamp output at the padded size; hr [B,3,Hs,Ws] (the image is the top-left corner).  Returns
    (loss: 0-d fp64, seed [B,3,Hp,Wp] fp64: 0 in the padding).  divisor defaults to the number of images (the mean)."""
    pre, hr = pre.double(), hr.double()
    Hs, Ws = hr.shape[-2:]
    sc = float(weight) / float(hr.shape[0] if divisor is None else divisor)
    loss, g, _, _ = value_and_grad(pre[..., :Hs, :Ws], hr, R, True, sc, sigma_n_sq)
    seed = torch.zeros_like(pre)
    seed[..., :Hs, :Ws] = g
    return loss, seed


def smooth(shape, seed: int = 0) -> torch.Tensor:
    """Smoothed uniform noise in [0, 1], fp64."""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    u = torch.rand(B * C, 1, H + 4, W + 4, generator=g, dtype=torch.float64)
    y = F.conv2d(u, torch.ones(1, 1, 5, 5, dtype=torch.float64) / 25.0).view(B, C, H, W)
    return (y - y.min()) / (y.max() - y.min())


def mixed_pair(shape, seed: int = 0, R: float = 1.0, sigma: float = 0.1):
    """(x, y) float32 built so that every branch of the map is taken with a margin: y = R * smoothed noise with an exactly constant
    20 x 20 patch in the bottom-right corner (b = 0 under the windows inside it: dead entries); x = 0.5 * y on the left 20 columns
    (exact in fp32: sv_raw ~ 0.25 EPS, the clamped branch); x = y + R * sigma * randn on the rest (the open branch; a share of it
    lies outside [0, R])."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed + 1000)
    y = smooth(shape, seed)
    y[..., H - 20:, W - 20:] = 0.5
    y = (y * R).float()
    x = (y.double() + R * sigma * torch.randn(shape, generator=g, dtype=torch.float64)).float()
    x[..., :, :20] = 0.5 * y[..., :, :20]
    return x.contiguous(), y.contiguous()
