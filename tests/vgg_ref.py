"""fp64 restatement of the VGG19 feature loss (include/m2t_perceptual.h) in torch on the CPU, for the tests of the HIP tower.

* ``forward_exact``     the tower in fp64 on the unrounded weights.
* ``forward_emulated``  the same with the kernels' rounding points: weights rounded to bf16 once, the normalised input in fp32, every
                        stored activation rounded to bf16 once (after bias and ReLU); the accumulation stays fp64.
* ``backward``          the TEACHER-FORCED input gradient: ReLU masks, pool arg-maxes and the signs of the criterion are taken from the
                        activations it is handed (the device's own, or an emulation's), so the map from the seeds to the gradient is
                        linear and a comparison is sharp.  ``rounded=False`` is exact fp64 on the unrounded weights; ``rounded=True``
                        uses the bf16 weights and rounds the gradient to bf16 where the kernels do (between layers, after the seed and
                        the mask).  ``fault=`` injects one-line mistakes for the gate's self-test.
* ``conv_gate`` / ``grad_gate``   the two gates.

The end-to-end gradient of this loss is discontinuous in the arithmetic (masks, arg-maxes and signs flip under rounding: a bf16
emulation is 13-18 % from fp64 autograd), which is why no test compares a kernel gradient with autograd of another forward pass.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

LAYERS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
CIN = (3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512)
COUT = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
LEVEL = (0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4)
TAP_LAYERS = (0, 2, 4, 8, 12)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
MARGIN = 3.0          # the project's rule (tests/attn_ref.py): a kernel may be 3 x as far from fp64 as the emulation of its arithmetic
KINDS = {"l1": (0, 0.0), "sl1": (3, 1.0), "l2": (1, 0.0)}


def pool_before(l):
    return l > 0 and LEVEL[l] != LEVEL[l - 1]


def bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def random_weights(seed):
    """He-initialised weights and small biases, float32, torchvision vgg19 names."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, ci, co in zip(LAYERS, CIN, COUT):
        sd[f"features.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f"features.{i}.bias"] = torch.randn(co, generator=g) * 0.05
    return sd


def weight_list(sd, rounded):
    ws = [sd[f"features.{i}.weight"].double() for i in LAYERS]
    bs = [sd[f"features.{i}.bias"].double() for i in LAYERS]
    return ([bf16(w) for w in ws] if rounded else ws), bs


def normalise(x, R, clamp, fp32):
    """[B,C,H,W] -> [B,3,H,W] float64; fp32=True evaluates (c(x) / R - mean) / std in float32, operation for operation as the kernel."""
    t = x.float() if fp32 else x.double()
    if clamp:
        t = t.clamp(0.0, R)
    if t.shape[1] == 1:
        t = t.repeat(1, 3, 1, 1)
    dt = t.dtype
    m = torch.tensor(MEAN, dtype=dt).view(1, 3, 1, 1)
    s = torch.tensor(STD, dtype=dt).view(1, 3, 1, 1)
    return ((t / torch.tensor(R, dtype=dt) - m) / s).double()


def _tower(a, ws, bs, rounded):
    acts = []
    for l in range(13):
        if pool_before(l):
            a = F.max_pool2d(a, 2)
        a = F.relu(F.conv2d(a, ws[l], bs[l], padding=1))
        if rounded:
            a = bf16(a)
        acts.append(a)
    return acts


def forward_exact(x, sd, R=1.0, clamp=False):
    ws, bs = weight_list(sd, False)
    return _tower(normalise(x, R, clamp, False), ws, bs, False)


def forward_emulated(x, sd, R=1.0, clamp=False):
    ws, bs = weight_list(sd, True)
    return _tower(normalise(x, R, clamp, True), ws, bs, True)


def rho(d, crit):
    if crit == "l1":
        return d.abs()
    if crit == "l2":
        return d * d
    ad = d.abs()
    return torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)          # sl1, beta = 1


def rho_prime(d, crit):
    if crit == "l1":
        return torch.sign(d)
    if crit == "l2":
        return 2.0 * d
    return torch.where(d.abs() < 1.0, d, torch.sign(d))


def loss_from_taps(xt, yt, tap_w, crit, scale=1.0):
    """scale * sum_k w_k mean(rho(F_k(x) - F_k(y))) and the five means, float64."""
    means = [rho(a - b, crit).mean() for a, b in zip(xt, yt)]
    return scale * sum(w * m for w, m in zip(tap_w, means)), means


def dgrad(g, w, fault=None):
    """the data gradient of a stride-1 3 x 3 convolution with padding 1: a convolution with the flipped, transposed taps"""
    wt = w.transpose(0, 1)
    if fault != "no_flip":
        wt = wt.flip(2, 3)
    if fault == "drop_tap":
        wt = wt.clone()
        wt[:, :, 0, 1] = 0.0
    return F.conv2d(g, wt, padding=1)


def pool_backward(a, g, last=False):
    """the gradient of the 2 x 2 stride-2 floor max pool of `a` to the FIRST maximum of each window in row-major order (as torch);
    last=True is the fault"""
    Ho, Wo = a.shape[2] // 2, a.shape[3] // 2
    win = torch.stack([a[:, :, dy:2 * Ho:2, dx:2 * Wo:2] for dy in (0, 1) for dx in (0, 1)])
    idx = 3 - torch.argmax(win.flip(0), dim=0) if last else torch.argmax(win, dim=0)
    gin = torch.zeros_like(a)
    k = 0
    for dy in (0, 1):
        for dx in (0, 1):
            gin[:, :, dy:2 * Ho:2, dx:2 * Wo:2] = g * (idx == k)
            k += 1
    return gin


def backward(acts, ytaps, sd, x, crit="l1", tap_w=(1.0,) * 5, scale=1.0, R=1.0, clamp=False, rounded=False, fault=None):
    """The teacher-forced gradient of the term with respect to x [B,C,H,W] (float64), from the saved post-ReLU activations `acts`
    (13 tensors [B,C_l,H_l,W_l]) of the x half and the five taps of the y half."""
    ws, _ = weight_list(sd, rounded)
    rnd = bf16 if rounded else (lambda t: t)

    def seed(k):
        a, b = acts[TAP_LAYERS[k]], ytaps[k]
        return (scale * tap_w[k] / a.numel()) * rho_prime(a - b, crit)

    g = rnd(seed(4) * (acts[12] > 0))
    for l in range(12, 0, -1):
        gi = dgrad(g, ws[l], fault)
        if pool_before(l):
            g = pool_backward(acts[l - 1], rnd(gi), last=(fault == "pool_last")) * (acts[l - 1] > 0)
        else:
            if (l - 1) in TAP_LAYERS and not (fault == "no_seed" and l - 1 == 2):
                gi = gi + seed(TAP_LAYERS.index(l - 1))
            mask_from = acts[l] if (fault == "wrong_mask" and acts[l].shape == acts[l - 1].shape) else acts[l - 1]
            g = rnd(gi * (mask_from > 0))
    g3 = dgrad(g, ws[0], fault)
    std = torch.tensor([1.0, 1.0, 1.0] if fault == "no_std" else STD, dtype=torch.float64).view(1, 3, 1, 1)
    g3 = g3 / (std * R)
    gx = g3.sum(1, keepdim=True) if x.shape[1] == 1 else g3
    if clamp:
        gx = gx * ((x.double() >= 0) & (x.double() <= R))
    return gx


FAULTS = ("no_flip", "drop_tap", "wrong_mask", "pool_last", "no_seed", "no_std")


def grad_gate(gx, exact, emulated):
    """(passes, error, budget): max |gx - exact| <= MARGIN * max |emulated - exact|, both relative to max |exact|"""
    ref = exact.abs().max().item()
    err = (gx.double() - exact).abs().max().item() / ref
    budget = MARGIN * (emulated - exact).abs().max().item() / ref
    return err <= budget, err, budget


def conv_bound(a, w, b, K):
    """2 K 2^-24 (|a| (*) |w| + |b|): the fp32 accumulation bound of a K-term dot product, elementwise"""
    mag = F.conv2d(a.abs(), w.abs(), None if b is None else b.abs(), padding=1)
    return 2.0 * K * 2.0 ** -24 * mag


def conv_gate(out, ref, bound):
    """elementwise |out - ref| <= 2^-8 |ref| + bound (one bf16 ulp of the output plus the accumulation bound); returns the worst ratio"""
    ratio = (out.double() - ref).abs() / (2.0 ** -8 * ref.abs() + bound + 1e-300)
    return ratio.max().item()
