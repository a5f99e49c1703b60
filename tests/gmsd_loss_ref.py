"""The fp64 restatement of the GMSD loss term (include/m2t_gmsd.h) in explicit torch ops, on the CPU: the yardstick of
tests/test_gmsd_loss_cpu.py and tests/test_gpu_gmsd_loss.py.  Nothing here goes through autograd: the gradient is the closed form of
the header, with its two conventions -- an entry with m = 0 adds nothing (torch gives 0 * inf = NaN there) and an image with
GMSD_b = 0 has no gradient at all.  The Prewitt pair takes the differences first, so a flat region gives exactly 0."""
import torch

T = 170.0 / 255.0 ** 2
LUMA = (0.299, 0.587, 0.114)


def _luminance(t, R):
    """[B,C,H,W] fp64 -> [B,H,W]: (0.299 r + 0.587 g + 0.114 b) / R, or the one channel / R."""
    if t.shape[1] == 3:
        return ((LUMA[0] * t[:, 0] + LUMA[1] * t[:, 1]) + LUMA[2] * t[:, 2]) / R
    assert t.shape[1] == 1
    return t[:, 0] / R


def _pool(l):
    """2 x 2 average with the zero pad to an even size: [B,H,W] -> [B,ceil(H/2),ceil(W/2)]."""
    B, H, W = l.shape
    p = torch.zeros((B, H + H % 2, W + W % 2), dtype=l.dtype)
    p[:, :H, :W] = l
    return ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + (p[:, 1::2, 0::2] + p[:, 1::2, 1::2])) * 0.25


def _prewitt(u):
    """(gx, gy) of [B,hp,wp], zero padding, differences first."""
    B, h, w = u.shape
    p = torch.zeros((B, h + 2, w + 2), dtype=u.dtype)
    p[:, 1:-1, 1:-1] = u
    def at(dy, dx):
        return p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = ((at(-1, 1) - at(-1, -1)) + (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1))) / 3.0
    gy = ((at(1, -1) - at(-1, -1)) + (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1))) / 3.0
    return gx, gy


def _prewitt_adjoint(ax, ay):
    """The adjoint of _prewitt applied to (a_x, a_y): [B,hp,wp]."""
    B, h, w = ax.shape
    out = torch.zeros((B, h + 2, w + 2), dtype=ax.dtype)
    def add(dy, dx, val):
        out[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] += val
    for dy in (-1, 0, 1):
        add(dy, 1, ax / 3.0)
        add(dy, -1, -ax / 3.0)
    for dx in (-1, 0, 1):
        add(1, dx, ay / 3.0)
        add(-1, dx, -ay / 3.0)
    return out[:, 1:-1, 1:-1]


def value_and_grad(x, y, R=1.0, clamp=False, scale=None, min_gmsd=None):
    """x, y [B,C,H,W] (any float dtype; widened to fp64) -> (value, gradient [B,C,H,W] fp64, GMSD_b [B] fp64, shares): value =
    scale * sum_b GMSD_b (scale = 1 / B by default), its gradient with respect to x, and the shares of the map entries of x that are
    dead (m = 0), of the elements of x the clamp holds back, and of those it lets through.  min_gmsd: assert GMSD_b >= it."""
    x, y = x.double(), y.double()
    B, C, H, W = x.shape
    if scale is None:
        scale = 1.0 / B
    R = float(R)
    xc = x.clamp(0.0, R) if clamp else x
    u, v = _pool(_luminance(xc, R)), _pool(_luminance(y, R))
    gx, gy = _prewitt(u)
    hx, hy = _prewitt(v)
    m, mp = torch.sqrt(gx * gx + gy * gy), torch.sqrt(hx * hx + hy * hy)
    D = m * m + mp * mp + T
    s = (2.0 * m * mp + T) / D
    d = (m - mp) ** 2 / D
    n = float(d.shape[1] * d.shape[2])
    mean_d = d.sum(dim=(1, 2), keepdim=True) / n
    var = ((d * d).sum(dim=(1, 2), keepdim=True) / n - mean_d * mean_d).clamp(min=0.0)
    gm = torch.sqrt(var)                                       # [B,1,1]
    if min_gmsd is not None:
        assert float(gm.min()) >= min_gmsd, gm.flatten().tolist()
    live = m > 0
    rho = torch.where(live, mp / torch.where(live, m, torch.ones_like(m)), torch.zeros_like(m))
    safe = torch.where(gm > 0, gm, torch.ones_like(gm))
    k = torch.where(gm > 0, (mean_d - d) / (n * safe), torch.zeros_like(d))      # s_i - mu = mean_d - d_i
    a = torch.where(live, k * 2.0 * (rho - s) / D, torch.zeros_like(m))
    du = _prewitt_adjoint(a * gx, a * gy)
    up = du.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]
    w = torch.tensor(LUMA if C == 3 else (1.0,), dtype=torch.float64).view(1, C, 1, 1)
    grad = scale * 0.25 * w / R * up.unsqueeze(1)
    inside = (x >= 0.0) & (x <= R)
    if clamp:
        grad = grad * inside
    shares = {"dead": float((~live).double().mean()), "clamped": float((~inside).double().mean()), "open": float(inside.double().mean())}
    return scale * gm.sum(), grad, gm.flatten(), shares


def mixed_pair(shape, seed=0, R=1.0):
    """(x, y) float32 [B,C,H,W] that hold every class of entry: a sector exactly 0 in both images (the black mask of an ultrasound
    frame: dead entries), a patch flat and non-zero in x only, a patch flat in y only, about 5 % of x outside [0, R], noise of about
    0.1 R elsewhere."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g) * 0.6 + 0.2
    x = y + 0.1 * torch.randn(shape, generator=g)
    out = torch.rand(shape, generator=g) < 0.05
    x = torch.where(out, torch.where(torch.rand(shape, generator=g) < 0.5, -0.2 * torch.ones(shape), 1.2 * torch.ones(shape)) +
                    0.05 * torch.randn(shape, generator=g), x)
    h3, w3 = max(H // 3, 1), max(W // 3, 1)
    x[..., :h3, :w3] = 0.0                                     # the sector: exactly 0 in both
    y[..., :h3, :w3] = 0.0
    x[..., H - h3:, :w3] = 0.375                               # flat and non-zero in x only
    y[..., :h3, W - w3:] = 0.625                               # flat in y only
    return (x * R).float(), (y * R).float()


def sector(shape):
    """The elements of the sector of mixed_pair whose 2 x 2 cell has only sector cells around it: their gradient is exactly 0."""
    B, C, H, W = shape
    h3, w3 = max(H // 3, 1), max(W // 3, 1)
    m = torch.zeros(shape, dtype=torch.bool)
    # cells (py, px) with py + 1 <= (h3 // 2) - 1 and px likewise: the cell, and every neighbour of every entry that reads it, is 0
    ph, pw = h3 // 2 - 2, w3 // 2 - 2
    if ph > 0 and pw > 0:
        m[..., :2 * ph, :2 * pw] = True
    return m
