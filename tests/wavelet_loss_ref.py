"""The fp64 restatement of the wavelet-domain loss term (include/m2t_wavelet.h) in explicit torch ops, on the CPU: the yardstick of
tests/test_wavelet_loss_cpu.py and tests/test_gpu_wavelet_loss.py.  Nothing here goes through autograd: the gradient is the closed
form of the header -- the transposed passes from the coarsest level down.  Every tap sum runs k ascending from 0.0 with separate
multiply and add, as the kernels' do; a periodic pass is a sum of rolls."""
import math

import torch

HAAR = ((0.5, 0.5), (0.5, -0.5))
_S3 = math.sqrt(3.0)
_DB2_LO = ((1.0 + _S3) / 8.0, (3.0 + _S3) / 8.0, (3.0 - _S3) / 8.0, (1.0 - _S3) / 8.0)
DB2 = (_DB2_LO, tuple((-1.0) ** k * _DB2_LO[3 - k] for k in range(4)))
TRI = ((0.25, 0.5, 0.25), (-0.25, 0.5, -0.25))               # a non-orthogonal 3-tap pair
# an 8-tap pair (the db4 scaling filter to 8 digits, normalised to sum 1, and its alternating flip): the longest reach the kernels take
_T8 = (0.23037781, 0.71484657, 0.63088077, -0.02798377, -0.18703481, 0.03084138, 0.03288301, -0.01059740)
_T8_LO = tuple(v / sum(_T8) for v in _T8)
TAP8 = (_T8_LO, tuple((-1.0) ** k * _T8_LO[7 - k] for k in range(8)))
FILTERS = {"haar": HAAR, "db2": DB2, "tri": TRI, "tap8": TAP8}
MIN_COEF = 1e-9                                                # the conditioning gate of eps = 0


def default_weights(J):
    return [1.0] * (3 * J) + [0.0]


def _pass(t, f, s, dim, sign=1):
    """out[n] = sum_k f[k] * t[(n + sign k s) mod N] along dim."""
    acc = torch.zeros_like(t)
    for k, fk in enumerate(f):
        acc = acc + float(fk) * torch.roll(t, -sign * k * s, dims=dim)
    return acc


def swt2(d, lo, hi, J):
    """d [..., H, W] fp64 -> the 3 J + 1 bands (LH_1, HL_1, HH_1, ..., LH_J, HL_J, HH_J, LL_J), a list of tensors of d's shape."""
    bands, a = [], d
    for j in range(1, J + 1):
        s = 2 ** (j - 1)
        rl, rh = _pass(a, lo, s, -1), _pass(a, hi, s, -1)
        ll, lh = _pass(rl, lo, s, -2), _pass(rl, hi, s, -2)
        hl, hh = _pass(rh, lo, s, -2), _pass(rh, hi, s, -2)
        bands += [lh, hl, hh]
        a = ll
    return bands + [a]


def adjoint(psi, lo, hi, J):
    """The adjoint of swt2 applied to the 3 J + 1 planes psi (None: an absent band, which adds nothing)."""
    def add(p, q):
        return q if p is None else p if q is None else p + q

    def tp(t, f, s, dim):
        return None if t is None else _pass(t, f, s, dim, sign=-1)

    abar = psi[3 * J]
    for j in range(J, 0, -1):
        s = 2 ** (j - 1)
        lh, hl, hh = psi[3 * (j - 1):3 * j]
        rl = add(tp(abar, lo, s, -2), tp(lh, hi, s, -2))
        rh = add(tp(hl, lo, s, -2), tp(hh, hi, s, -2))
        abar = add(tp(rl, lo, s, -1), tp(rh, hi, s, -1))
    return abar


def rho(c, eps):
    return c.abs() if eps == 0 else torch.sqrt(c * c + eps * eps)


def rho_prime(c, eps):
    return torch.sign(c) if eps == 0 else c / torch.sqrt(c * c + eps * eps)


def difference(x, y, R, clamp):
    x, y = x.double(), y.double()
    iR = 1.0 / float(R)
    return (x.clamp(0.0, float(R)) if clamp else x) * iR - y * iR


def value_and_grad(x, y, R=1.0, clamp=False, scale=None, lo=HAAR[0], hi=HAAR[1], J=2, weights=None, eps=0.0, skip=()):
    """x, y [B,C,H,W] (any float dtype; widened to fp64) -> (value, gradient [B,C,H,W] fp64, band sums [3 J + 1] fp64 (0 for a band
    of weight 0), the smallest non-zero |c| of a weighted band).  scale = 1 / (B C H W) by default; skip: bands left out altogether
    (the comparison for a weight of 0).  For eps = 0 the conditioning is ASSERTED: every coefficient of a weighted band is either
    exactly 0 with nothing but zeros in its support, or has |c| >= MIN_COEF -- no element is left ungated."""
    B, C, H, W = x.shape
    if scale is None:
        scale = 1.0 / (B * C * H * W)
    weights = default_weights(J) if weights is None else [float(w) for w in weights]
    assert len(weights) == 3 * J + 1
    d = difference(x, y, R, clamp)
    bands = swt2(d, lo, hi, J)
    smallest = math.inf
    if eps == 0:
        ones = [1.0] * len(lo)
        support = swt2((d != 0).double(), ones, ones, J)       # > 0 where the coefficient's support holds a non-zero difference
        reach = [support[3 * (b // 3)] if b < 3 * J else support[3 * J] for b in range(3 * J + 1)]
    total, sums, psi = 0.0, [], []
    for b, (c, w) in enumerate(zip(bands, weights)):
        if w == 0.0 or b in skip:
            sums.append(0.0)
            psi.append(None)
            continue
        if eps == 0:
            zero = c == 0
            assert not bool((zero & (reach[b] > 0)).any()), f"band {b}: a coefficient cancels to exactly 0 on a non-zero support"
            assert not bool((~zero & (reach[b] == 0)).any())
            if bool((~zero).any()):
                m = float(c[~zero].abs().min())
                smallest = min(smallest, m)
                assert m >= MIN_COEF, f"band {b}: min non-zero |c| = {m:.3g} is below the conditioning gate (change the seed)"
        S = rho(c, eps).sum()
        sums.append(float(S))
        total = total + w * S
        psi.append(w * rho_prime(c, eps))
    abar = adjoint(psi, lo, hi, J)
    grad = (scale * (1.0 / float(R))) * abar
    if clamp:
        xd = x.double()
        grad = grad * ((xd >= 0.0) & (xd <= float(R)))
    return float(scale * total), grad, torch.tensor(sums, dtype=torch.float64), smallest


def mixed_pair(shape, seed=0, R=1.0, div=3):
    """(x, y) float32 [B,C,H,W]: a sector (the top-left H // div x W // div) exactly 0 in both images -- the black mask of an
    ultrasound frame --, about 5 % of x outside [0, R], noise of about 0.1 R elsewhere."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g) * 0.6 + 0.2
    x = y + 0.1 * torch.randn(shape, generator=g)
    out = torch.rand(shape, generator=g) < 0.05
    x = torch.where(out, torch.where(torch.rand(shape, generator=g) < 0.5, -0.2 * torch.ones(shape), 1.2 * torch.ones(shape)) +
                    0.05 * torch.randn(shape, generator=g), x)
    h3, w3 = H // div, W // div
    x[..., :h3, :w3] = 0.0
    y[..., :h3, :w3] = 0.0
    return (x * R).float(), (y * R).float()


def sector(shape, taps, J, div=3):
    """The elements of mixed_pair's sector whose whole reach lies in it: every coefficient they feed reads only zeros, so their
    gradient is exactly 0.  A pass at level j reaches (taps - 1) 2^(j-1) forward, the cascade (taps - 1) (2^J - 1)."""
    B, C, H, W = shape
    h3, w3 = H // div, W // div
    r = (taps - 1) * (2 ** J - 1)
    m = torch.zeros(shape, dtype=torch.bool)
    if h3 - r > r and w3 - r > r:
        m[..., r:h3 - r, r:w3 - r] = True
    return m
