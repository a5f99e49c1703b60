"""MATLAB-style ``imresize(..., 'bicubic')`` by an integer factor 2, 3 or 4 on the device (include/m2t_resize.h, k_resize.hip):
down with antialiasing, up without; mirrored borders with the edge pixel repeated; rows first, then columns, in fp64.

What it stands in for: the reference trains and validates on LR folders produced offline by MATLAB (``US1K_train_LR_bicubic``,
datas/us1k.py:84,176; ``<LR_folder>/X{s}`` of datas/benchmark.py), and its result tables open with a "Bicubic" row.  `datas.US1K` /
`datas.Benchmark` synthesise their LR half with `imresize_u8` when no LR is given, `tools/make_lr.py` writes the folders, and
`BicubicUp` is the baseline row under `metrics.evaluate`.

Parity with MATLAB itself is unpinned (no MATLAB and no file of the dataset where this is built), as for `piq` / `pytorch_msssim`
(DESIGN.md §7); the definition is pinned by tests/imresize_ref.py (MATLAB's general contributions form in numpy fp64) and, away
from the borders, by torch's antialiased bicubic interpolation.  Device tensors only: there is no host fallback."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

SCALES = (2, 3, 4)
# first tap of the dense filter relative to cell q (down: input q * s + m; up: input q + m), and the number of taps per phase
FIRST_TAP = {(2, False): -3, (3, False): -4, (4, False): -6, (2, True): -2, (3, True): -2, (4, True): -2}
NUM_TAPS = {(2, False): 8, (3, False): 11, (4, False): 16, (2, True): 5, (3, True): 5, (4, True): 5}


def _cubic(x: float) -> float:
    # cubic convolution kernel, a = -0.5; the expression order is the one of the host code in k_resize.hip
    x = abs(x)
    if x <= 1.0:
        return (1.5 * x - 2.5) * x * x + 1.0
    if x <= 2.0:
        return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0
    return 0.0


def filter_taps(scale: int, up: bool = False) -> np.ndarray:
    """The normalised fp64 weights the kernels receive in their arguments, [phases, taps] (pure host code, the same IEEE operations
    in the same order as the library's host side).

    down: one phase; tap t weighs input ``i * scale + FIRST_TAP + t`` of output i (8 / 11 / 16 taps; x3 holds two exact zeros,
    9 non-zero).  up: `scale` phases; tap t of phase p weighs input ``q + FIRST_TAP + t`` of output ``q * scale + p`` (five taps:
    the four of the phase and an exact zero at one end)."""
    if scale not in SCALES:
        raise ValueError(f"scale must be one of {SCALES}, got {scale}")
    up = bool(up)
    m0, nt = FIRST_TAP[(scale, up)], NUM_TAPS[(scale, up)]
    out = np.zeros((scale if up else 1, nt), dtype=np.float64)
    for p in range(out.shape[0]):
        w, total = [], 0.0
        for t in range(nt):
            m = m0 + t
            # u - j from its exact integer numerator over 2 s: one rounding
            v = _cubic((2 * p + 1 - scale - 2 * scale * m) / (2.0 * scale)) if up else _cubic((scale - 1 - 2 * m) / (2.0 * scale)) / scale
            w.append(v)
            total += v
        out[p] = [v / total for v in w]
    return out


def _out_side(n: int, scale: int, up: bool) -> int:
    return n * scale if up else n // scale


def imresize_u8(img: torch.Tensor, scale: int, up: bool = False, out: torch.Tensor = None) -> torch.Tensor:
    """uint8 [H,W,3] on the device -> uint8 [H',W',3]: the fp64 result rounded half away from zero and saturated.  `out`: an
    optional contiguous uint8 destination of H' * W' * 3 elements (a slot of a pool)."""
    if img.dtype != torch.uint8 or img.dim() != 3 or not img.is_cuda or not img.is_contiguous():
        raise _lib.M2TError(f"imresize_u8 takes a contiguous uint8 [H,W,3] device tensor, got {img.dtype} {tuple(img.shape)} on {img.device}")
    H, W, C = img.shape
    oh, ow = _out_side(H, scale, up), _out_side(W, scale, up)
    if out is None:
        out = torch.empty(max(oh, 0), max(ow, 0), C, dtype=torch.uint8, device=img.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.device != img.device or out.numel() != oh * ow * C:
        raise _lib.M2TError("imresize_u8: `out` must be a contiguous uint8 tensor of H' * W' * 3 elements on the image's device")
    lib = _lib.load()
    with torch.cuda.device(img.device):
        _lib.check(lib.m2t_imresize_u8(_lib.ptr(img), H, W, C, _lib.ptr(out), int(scale), int(bool(up)), _lib.stream_ptr()),
                   "m2t_imresize_u8")
    return out


def imresize(x: torch.Tensor, scale: int, up: bool = False, clamp_max: float = 0.0) -> torch.Tensor:
    """float32 [N,C,H,W] on the device -> float32 [N,C,H',W']: the fp64 result rounded once to fp32, clamped to [0, clamp_max]
    first when clamp_max > 0."""
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda:
        raise _lib.M2TError(f"imresize takes a float32 [N,C,H,W] device tensor, got {x.dtype} {tuple(x.shape)} on {x.device}")
    x = x.contiguous()
    N, C, H, W = x.shape
    out = torch.empty(N, C, max(_out_side(H, scale, up), 0), max(_out_side(W, scale, up), 0), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(lib.m2t_imresize_f32(_lib.ptr(x), N * C, H, W, _lib.ptr(out), int(scale), int(bool(up)), float(clamp_max),
                                        _lib.stream_ptr()), "m2t_imresize_f32")
    return out


def imresize_adjoint(g: torch.Tensor, scale: int) -> torch.Tensor:
    """The adjoint D^T of the bicubic down-sampler (include/m2t_consistency.h): float32 [N,C,h,w] on the device -> float32
    [N,C,h*scale,w*scale] with ``<imresize(x, scale), g> = <x, imresize_adjoint(g, scale)>``; the mirrored border makes it more than a
    transposed stencil (border pixels also receive the reflected taps).  The fp64 result is rounded once to fp32."""
    if g.dtype != torch.float32 or g.dim() != 4 or not g.is_cuda:
        raise _lib.M2TError(f"imresize_adjoint takes a float32 [N,C,h,w] device tensor, got {g.dtype} {tuple(g.shape)} on {g.device}")
    g = g.contiguous()
    N, C, h, w = g.shape
    out = torch.empty(N, C, h * int(scale), w * int(scale), dtype=torch.float32, device=g.device)
    lib = _lib.load()
    with torch.cuda.device(g.device):
        _lib.check(lib.m2t_imresize_adjoint_f32(_lib.ptr(g), N * C, h, w, _lib.ptr(out), int(scale), 0, _lib.stream_ptr()),
                   "m2t_imresize_adjoint_f32")
    return out


class BicubicUp:
    """The interpolation baseline as a callable ``lr -> sr`` (clamped to [0, rgb_range]), usable as `model` of `metrics.evaluate`:
    the "Bicubic" row of a results table is ``evaluate(BicubicUp(s), pairs, s, ...)``.

    The float path goes from the LR tensor to the SR tensor in one rounding: it skips the 8-bit re-quantisation that a baseline
    image saved to a file and read back carries, so its PSNR is a little above such a table row's."""

    def __init__(self, scale: int, rgb_range: float = 1.0):
        if scale not in SCALES:
            raise ValueError(f"scale must be one of {SCALES}, got {scale}")
        if not (math.isfinite(rgb_range) and rgb_range > 0):
            raise ValueError("rgb_range must be a finite number > 0")
        self.scale, self.rgb_range = scale, float(rgb_range)

    def __call__(self, lr: torch.Tensor) -> torch.Tensor:
        return imresize(lr, self.scale, up=True, clamp_max=self.rgb_range)


def modcrop(img: np.ndarray, scale: int) -> np.ndarray:
    """The top-left (H - H mod s) x (W - W mod s) part of an HWC image (what the dataset scripts do before imresize, and the crop
    datas/benchmark.py applies to HR afterwards)."""
    return img[:img.shape[0] - img.shape[0] % scale, :img.shape[1] - img.shape[1] % scale]
