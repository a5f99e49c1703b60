"""fp64 restatement of the frequency-domain loss term (k_fft_loss.hip; include/m2t_spectral.h), for the tests only.

    x = clamp(pre, 0, R) / R,  y = hr / R,  d = x - y,  D = s * rfft2(d)   (s = 1 "backward", 1 / sqrt(H W) "ortho")
    value = scale * sum(|Re D| + |Im D|)            (scale = 1 / (2 B C H (W/2+1)) for the mean)
    d value / d pre(h, w) = scale / R * s * Re sum_ky sum_{kx <= W/2} (Sr + i Si) e^{+2 pi i (ky h / H + kx w / W)}

with Sr = sign(Re D), Si = sign(Im D), sign(0) = 0, and the imaginary part of the four self-conjugate bins (ky in {0, H/2}, kx in
{0, W/2}) exactly 0.  The value comes from torch.fft in fp64; the gradient from the FORMULA (explicit DFT matrices with integer
phase reduction), not from autograd -- tests/test_fft_loss_cpu.py compares the two.  Inputs are the kernel's fp32 inputs, widened.
"""
import math

import torch

NORMS = {"backward": 0, "ortho": 1}


def norm_factor(norm, H, W):
    assert norm in NORMS, norm
    return 1.0 / math.sqrt(H * W) if norm == "ortho" else 1.0


def self_conjugate_mask(H, W):
    """[H, W/2+1] bool: the bins whose imaginary part is mathematically 0."""
    m = torch.zeros(H, W // 2 + 1, dtype=torch.bool)
    for ky in (0, H // 2):
        for kx in (0, W // 2):
            m[ky, kx] = True
    return m


def spectrum(d, norm="backward"):
    """s * rfft2(d) in fp64 with the imaginary part of the self-conjugate bins forced to 0: complex [..., H, W/2+1]."""
    d = d.double()
    H, W = d.shape[-2:]
    D = torch.fft.rfft2(d) * norm_factor(norm, H, W)
    im = D.imag.clone()
    im[..., self_conjugate_mask(H, W)] = 0.0
    return torch.complex(D.real.clone(), im)


def _phases(n, rows, cols):
    """e^{+2 pi i r c / n} for r < rows, c < cols, the angle reduced in integers first: [rows, cols] complex128."""
    k = (torch.arange(rows).view(-1, 1) * torch.arange(cols).view(1, -1)) % n
    ang = 2.0 * math.pi * k.double() / n
    return torch.complex(torch.cos(ang), torch.sin(ang))


def adjoint_of_signs(D):
    """Re sum_ky sum_{kx <= W/2} (sign Re D + i sign Im D) e^{+2 pi i (ky h / H + kx w / W)}: [..., H, W] from D [..., H, W/2+1]
    (W is taken as 2 * (W/2+1) - 2: even).  The half spectrum, no Hermitian doubling."""
    H, Wh = D.shape[-2:]
    W = 2 * (Wh - 1)
    S = torch.complex(torch.sign(D.real), torch.sign(D.imag))
    Eh = _phases(H, H, H)            # [h, ky]
    Ew = _phases(W, Wh, W)           # [kx, w]
    return (Eh @ S @ Ew).real


def value_and_grad(x, y, data_range=1.0, clamp=False, scale=None, norm="backward"):
    """(value, d value / dx) for x, y [B,C,H,W] (any float dtype; widened), both fp64.  scale defaults to 1 / reals (the mean)."""
    x, y = x.double(), y.double()
    R = float(data_range)
    B, C, H, W = x.shape
    if scale is None:
        scale = 1.0 / (2 * B * C * H * (W // 2 + 1))
    xn = (x.clamp(0.0, R) if clamp else x) / R
    D = spectrum(xn - y / R, norm)
    value = scale * (D.real.abs().sum() + D.imag.abs().sum())
    grad = scale / R * norm_factor(norm, H, W) * adjoint_of_signs(D)
    if clamp:
        grad = grad * ((x >= 0.0) & (x <= R)).double()
    return value, grad


def loss_and_seed(pre, hr, weight=1.0, divisor=None, R=1.0, norm="backward"):
    """What m2t_fft_loss adds: pre [B,3,Hp,Wp] the pre-clamp output (padded), hr [B,3,Hs,Ws].  Returns (loss, seed [B,3,Hp,Wp]) with
    the seed exactly 0 in the padding and where the clamp is active.  divisor defaults to the number of reals of this batch."""
    B, C, Hs, Ws = hr.shape
    if divisor is None:
        divisor = 2 * B * C * Hs * (Ws // 2 + 1)
    value, g = value_and_grad(pre[..., :Hs, :Ws], hr, R, True, weight / divisor, norm)
    seed = torch.zeros(pre.shape, dtype=torch.float64)
    seed[..., :Hs, :Ws] = g
    return value, seed


def kink_margin(d):
    """The smallest |component| of the fp64 spectrum of d over the non-self-conjugate components, divided by the RMS over those
    components.  The gradient of the L1 is discontinuous where a component crosses 0: tests keep this >= 1e-5."""
    D = spectrum(d, "backward")
    H, W = d.shape[-2:]
    sc = self_conjugate_mask(H, W)
    comps = torch.cat([D.real.reshape(-1), D.imag[..., ~sc].reshape(-1)])
    return float(comps.abs().min() / comps.pow(2).mean().sqrt())


def inputs(H, W, seed, B=2, C=3, push_seed=None):
    """The issue's recipe: x uniform, y = (x + 0.1 randn).clamp(0, 1), both cast to fp32.  With push_seed, about 10 % of x is pushed
    outside [0, 1] (half below, half above) -- before any precondition is evaluated."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g, dtype=torch.float64)
    y = (x + 0.1 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    if push_seed is not None:
        g2 = torch.Generator().manual_seed(push_seed)
        pick = torch.rand(B, C, H, W, generator=g2, dtype=torch.float64) < 0.1
        low = torch.rand(B, C, H, W, generator=g2, dtype=torch.float64) < 0.5
        off = 0.05 + 0.3 * torch.rand(B, C, H, W, generator=g2, dtype=torch.float64)
        x = torch.where(pick, torch.where(low, -off, 1.0 + off), x)
    return x.float(), y.float()


def torch_fp32_floor(x, y, clamp=False):
    """Errors of torch's OWN fp32 pipeline against this fp64 reference on the same fp32 inputs: (spectrum, value, gradient) --
    spectrum and gradient as max-abs over the reference's max-abs, the value relative."""
    H, W = x.shape[-2:]
    want_v, want_g = value_and_grad(x, y, 1.0, clamp)
    xn = (x.clamp(0.0, 1.0) if clamp else x).float()
    want_D = spectrum(xn.double() - y.double())
    leaf = x.float().clone().requires_grad_(True)
    d32 = (leaf.clamp(0.0, 1.0) if clamp else leaf) - y.float()
    D32 = torch.view_as_real(torch.fft.rfft2(d32))
    keep = torch.ones(H, W // 2 + 1, 2)
    keep[..., 1][self_conjugate_mask(H, W)] = 0.0
    D32 = D32 * keep
    v32 = D32.abs().mean()
    v32.backward()
    want_Dr = torch.view_as_real(want_D)
    e_spec = float((D32.detach().double() - want_Dr).abs().max() / want_Dr.abs().max())
    e_val = abs(float(v32.detach()) - float(want_v)) / abs(float(want_v))
    e_grad = float((leaf.grad.double() - want_g).abs().max() / want_g.abs().max())
    return e_spec, e_val, e_grad
