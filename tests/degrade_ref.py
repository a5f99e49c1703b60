"""NumPy fp64 restatement of include/m2t_degrade.h for the tests: the kernel bank, the symmetric folding, the tap loop in the stated
order (rows outer, columns inner, from 0.0, separate multiply and add), Philox4x32-10 in uint64 arithmetic, the Irwin-Hall variate,
the value with one rounding per operation, the quantisation and the flips of crop_patch.  Written from the definition, vectorised
over pixels (NumPy never fuses a multiply with an add), not from the kernel text."""
import math
import random

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


# ------------------------------------------------------------------------------------------------------------- the bank
def kernel(K, s1, s2, theta):
    """Sigma = Q diag(s1^2, s2^2) Q^T, [[a, b], [b, c]] = Sigma^-1, w[i][j] ~ exp(-(a oj^2 + 2 b oj oi + c oi^2) / 2), / its sum."""
    Q = np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])
    P = np.linalg.inv(Q @ np.diag([s1 * s1, s2 * s2]) @ Q.T)
    a, b, c = P[0, 0], P[0, 1], P[1, 1]
    w = np.empty((K, K))
    for i in range(K):
        for j in range(K):
            oi, oj = i - (K - 1) / 2, j - (K - 1) / 2
            w[i, j] = math.exp(-0.5 * (a * oj * oj + 2 * b * oj * oi + c * oi * oi))
    return w / w.sum()


def default_ksize(s, sigma_max):
    top = 21 if s % 2 else 20
    for K in range(1 if s % 2 else 2, top + 1, 2):
        if K >= 6 * sigma_max + 1:
            return K
    return top


def bank(s, M=256, sigma=None, iso_prob=0.5, K=None, seed=33):
    """(kernels [M, K, K], the random.Random after the bank's draws)."""
    sigma = (0.2, 0.8 * s) if sigma is None else sigma
    K = default_ksize(s, sigma[1]) if K is None else K
    rng = random.Random(seed)
    out = []
    for _ in range(M):
        iso = rng.random() < iso_prob
        s1 = rng.uniform(*sigma)
        s2 = s1 if iso else rng.uniform(*sigma)
        out.append(kernel(K, s1, s2, rng.uniform(0, math.pi)))
    return np.stack(out), rng


# ------------------------------------------------------------------------------------------------------------- blur + decimate
def fold(i, N):
    """Repeated symmetric folding: -1 -> 0, -2 -> 1, N -> N - 1, N + 1 -> N - 2, ... until the index is inside."""
    i = int(i)
    while i < 0 or i >= N:
        i = -1 - i if i < 0 else 2 * N - 1 - i
    return i


def first_tap(s, X, K):
    assert (s - K) % 2 == 0
    return s * X + (s - K) // 2


def blur_decimate(hr, w, s, ly, lx, lh, lw):
    """acc [lh, lw, C] fp64 of the LR pixels (ly .. ly + lh, lx .. lx + lw) in LR-image coordinates."""
    H, W, C = hr.shape
    K = w.shape[0]
    rows = np.array([[fold(first_tap(s, ly + y, K) + i, H) for i in range(K)] for y in range(lh)])     # [lh, K]
    cols = np.array([[fold(first_tap(s, lx + x, K) + j, W) for j in range(K)] for x in range(lw)])     # [lw, K]
    src = hr.astype(np.float64)
    acc = np.zeros((lh, lw, C))
    for i in range(K):
        for j in range(K):
            p = w[i, j] * src[rows[:, i][:, None], cols[:, j][None, :], :]      # one rounding
            acc = acc + p                                                       # one rounding
    return acc


# ------------------------------------------------------------------------------------------------------------- noise
def philox4x32_10(c, k):
    """c: four uint32 arrays (as uint64), k: two Python ints -> four uint64 arrays holding uint32 words."""
    c0, c1, c2, c3 = [np.asarray(v, dtype=np.uint64) & MASK for v in c]
    k0, k1 = int(k[0]) & 0xFFFFFFFF, int(k[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        h0, l0, h1, l1 = p0 >> S32, p0 & MASK, p1 >> S32, p1 & MASK
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def variate(c0, sel, ch, noise_id, seed):
    """g = (2 S + 12 - 12 * 2^32) / 2^33 with S the integer sum of the twelve words of the blocks j = 0, 1, 2."""
    c0 = np.asarray(c0, dtype=np.uint64)
    S = np.zeros(c0.shape, dtype=np.uint64)
    for j in range(3):
        one = np.ones(c0.shape, dtype=np.uint64)
        out = philox4x32_10((c0, one * np.uint64(3 * sel + j + 8 * ch), one * np.uint64(noise_id & 0xFFFFFFFF),
                             one * np.uint64((noise_id >> 32) & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        for v in out:
            S = S + v
    n = (np.uint64(2) * S + np.uint64(12)).astype(np.int64) - np.int64(12 << 32)
    return n.astype(np.float64) / float(1 << 33)


def quantise(acc, sigma_add, sigma_speckle, gray, noise_id, seed):
    """acc [h, w, C] -> uint8 [h, w, C]; c0 = y * w + x inside the item."""
    h, w, C = acc.shape
    c0 = (np.arange(h, dtype=np.uint64)[:, None] * np.uint64(w) + np.arange(w, dtype=np.uint64)[None, :]) & MASK
    out = np.empty((h, w, C), dtype=np.uint8)
    for c in range(C):
        ch = 0 if gray else c
        v = acc[:, :, c]
        if sigma_speckle != 0.0:
            t = sigma_speckle * variate(c0, 1, ch, noise_id, seed)
            t = t * acc[:, :, c]
            v = acc[:, :, c] + t
        if sigma_add != 0.0:
            u = sigma_add * variate(c0, 0, ch, noise_id, seed)
            v = v + u
        out[:, :, c] = np.minimum(np.maximum(np.rint(v), 0.0), 255.0).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------- entries
def flip(p, flags):
    """crop_patch's order on an HWC array: [:, ::-1], [::-1, :], transpose(1, 0, 2)."""
    if flags & 1:
        p = p[:, ::-1, :]
    if flags & 2:
        p = p[::-1, :, :]
    if flags & 4:
        p = p.transpose(1, 0, 2)
    return p


def to_tensor(p_u8):
    """HWC uint8 -> CHW float32 / 255 (one correctly rounded fp32 division)."""
    return np.ascontiguousarray(p_u8.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0)


def image_u8(hr, w, s, sigma_add=0.0, sigma_speckle=0.0, gray=True, noise_id=0, seed=33):
    """The whole image: uint8 [H // s, W // s, C]."""
    H, W, _ = hr.shape
    acc = blur_decimate(hr, w, s, 0, 0, H // s, W // s)
    return quantise(acc, sigma_add, sigma_speckle, gray, noise_id, seed)


def patch_u8(hr, w, s, lp, lx, ly, flags, sigma_add=0.0, sigma_speckle=0.0, gray=True, noise_id=0, seed=33):
    """(LR uint8 [lp, lp, C], HR uint8 [lp s, lp s, C]) after the flips; the item of the noise counter is the patch."""
    acc = blur_decimate(hr, w, s, ly, lx, lp, lp)
    q = quantise(acc, sigma_add, sigma_speckle, gray, noise_id, seed)
    return flip(q, flags), flip(hr[ly * s:(ly + lp) * s, lx * s:(lx + lp) * s, :], flags)


def patches(hr_images, kernels, s, lp, items, gray=True, seed=33):
    """items: (image index, lx, ly, flags, bank index, sigma_add, sigma_speckle, noise_id) -> (lr [n,C,lp,lp], hr [n,C,lp s,lp s]) float32."""
    lr, hr = [], []
    for img, lx, ly, flags, index, sa, ss, nid in items:
        a, b = patch_u8(hr_images[img], kernels[index], s, lp, lx, ly, flags, sa, ss, gray, nid, seed)
        lr.append(to_tensor(a))
        hr.append(to_tensor(b))
    return np.stack(lr), np.stack(hr)
