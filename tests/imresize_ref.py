"""fp64 restatement of MATLAB-style imresize(..., 'bicubic') by an integer factor (include/m2t_resize.h), for the tests only.

Deliberately NOT the kernel's formulation: the kernel applies one fixed filter per phase on `q * s + m`; this builds, per axis,
MATLAB's general per-output weight and index tables (`contributions`: kernel width 4 -- 4 s with antialiasing --, P = ceil(width)
+ 2 candidate taps from left = floor(u - width / 2), weights h(u - index) normalised by their row sum, indices folded through
aux = [1:n, n:-1:1], all-zero columns dropped) and resizes axis by axis, rows first.  The only liberty: the centre u is written
0-based for the integer factor (u = (i + 1/2) s - 1/2 down, (i + 1/2) / s - 1/2 up) instead of with a floating scale = 1 / s, so
that the down-scaling centres are exact, and the distance u - index is evaluated from its exact integer numerator.  Also the
quantiser (half away from zero, then saturate), the tie margin, and the inputs the CPU and GPU tests share.  Parity with MATLAB itself is unpinned (no MATLAB here)."""
import functools

import numpy as np

SCALES = (2, 3, 4)
SHAPES = [(1, 1), (1, 9), (5, 7), (37, 53), (70, 131)]       # (h, w) of the SMALLER image: down runs on (h s, w s), up on (h, w)


def cubic(x):
    """MATLAB's cubic(): the a = -0.5 cubic convolution kernel in its expanded polynomial form."""
    ax = np.abs(x)
    ax2, ax3 = ax * ax, ax * ax * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1.0) * (ax <= 1) + (-0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0) * ((1 < ax) & (ax <= 2))


def contributions(n: int, s: int, up: bool, fold: bool = True):
    """(weights [n_out, P'], indices [n_out, P'] 0-based) of one axis of length n.  fold=False leaves the indices unmirrored."""
    if up:
        n_out, width = n * s, 4.0
        u = (np.arange(n_out, dtype=np.float64) + 0.5) / s - 0.5
        h = cubic
    else:
        assert n % s == 0
        n_out, width = n // s, 4.0 * s
        u = (np.arange(n_out, dtype=np.float64) + 0.5) * s - 0.5
        h = lambda x: cubic(x / s) / s                                   # noqa: E731
    left = np.floor(u - width / 2.0)
    P = int(np.ceil(width)) + 2
    ind = left[:, None] + np.arange(P, dtype=np.float64)[None, :]
    # u - index from its exact integer numerator over 2 s, one rounding: written as u[:, None] - ind, the rounding of u (an absolute
    # error that grows with the position) moves the x3 up-scaling weights by up to 3e-14 on a 400-pixel axis, which is more than one
    # fp32 rounding of a result that cancels to 1e-7 of its terms
    i2 = 2.0 * np.arange(n_out, dtype=np.float64)[:, None]
    dist = (i2 + 1.0 - s - 2.0 * s * ind) / (2.0 * s) if up else (i2 * s + s - 1.0 - 2.0 * ind) / 2.0
    assert np.abs(dist - (u[:, None] - ind)).max() <= 1e-9
    w = h(dist)
    w = w / w.sum(axis=1, keepdims=True)
    ind = ind.astype(np.int64)
    keep = np.any(w != 0.0, axis=0)
    w, ind = w[:, keep], ind[:, keep]
    if fold:
        aux = np.concatenate([np.arange(n), np.arange(n - 1, -1, -1)])   # [1:n, n:-1:1], 0-based
        ind = aux[np.mod(ind, 2 * n)]
    return w, ind


def resize_axis(a: np.ndarray, axis: int, s: int, up: bool) -> np.ndarray:
    w, ind = contributions(a.shape[axis], s, up)
    a = np.moveaxis(a, axis, 0)
    out = np.zeros((w.shape[0],) + a.shape[1:], dtype=np.float64)
    for p in range(w.shape[1]):
        out += w[:, p].reshape((-1,) + (1,) * (a.ndim - 1)) * a[ind[:, p]]
    return np.moveaxis(out, 0, axis)


def imresize(a: np.ndarray, s: int, up: bool = False, axes=(0, 1)) -> np.ndarray:
    """fp64 result before any rounding; axes = (row axis, column axis): (0, 1) for HWC, (1, 2) / (2, 3) for planar stacks."""
    a = np.asarray(a, dtype=np.float64)
    return resize_axis(resize_axis(a, axes[0], s, up), axes[1], s, up)


def quantise(v: np.ndarray) -> np.ndarray:
    """Half away from zero, then saturate to [0, 255]."""
    t = np.trunc(v)
    r = t + np.sign(v) * (np.abs(v - t) >= 0.5)
    return np.clip(r, 0, 255).astype(np.uint8)


def tie_margin(v: np.ndarray) -> float:
    """Smallest distance of a pre-rounding value to a half-integer."""
    return float(np.min(np.abs(v - np.floor(v) - 0.5))) if v.size else 1.0


def modcrop(img: np.ndarray, s: int) -> np.ndarray:
    return np.ascontiguousarray(img[:img.shape[0] - img.shape[0] % s, :img.shape[1] - img.shape[1] % s])


# ----------------------------------------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def u8_cases(s: int, up: bool):
    """[(name, uint8 HWC input, pre-rounding fp64 reference)] for one factor and direction: every shape with both generators
    (np.random.default_rng(33 + s) uniform uint8, drawn in the order of SHAPES, and the oracle's closed-form image)."""
    from oracle.m2trans_oracle import closed_form_u8_image
    rng = np.random.default_rng(33 + s)
    out = []
    for h, w in SHAPES:
        H, W = (h, w) if up else (h * s, w * s)
        for name, img in (("rng", rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)), ("closed", closed_form_u8_image(H, W))):
            out.append((f"{name}{H}x{W}", img, imresize(img, s, up)))
    return out


@functools.lru_cache(maxsize=None)
def dataset_images(s: int):
    """Five HR images of different sizes for the dataset tests, two of them no multiple of s, with the reference LR of their
    mod-cropped part: [(hr, hr_modcropped, pre-rounding LR, quantised LR)]."""
    from oracle.m2trans_oracle import closed_form_u8_image
    extra = [(0, 0), (1, s - 1), (0, 0), (s - 1, 1), (0, 0)]
    out = []
    for i, (dh, dw) in enumerate(extra):
        hr = closed_form_u8_image((30 + 3 * i) * s + dh, (41 + 2 * i) * s + dw, phase=0.2 * i)
        crop = modcrop(hr, s)
        v = imresize(crop, s, False)
        out.append((hr, crop, v, quantise(v)))
    return out
