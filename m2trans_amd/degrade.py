"""LR synthesis beyond bicubic (include/m2t_degrade.h, k_degrade.hip): the classical degradation model
`LR = ((HR (*) k) downsampled by s) * (1 + n_s) + n_a` with the blur kernel `k` and the two noise levels drawn per sample.

The reference trains on MATLAB-bicubic pairs only and carries its noise augmentation as dead code (datas/us1k.py:156-167).  A
`Degradation` holds a bank of anisotropic Gaussian kernels (or measured PSFs handed in as an array), built on the host in fp64 and
uploaded once, and a `random.Random` of its own for the per-sample draws, so that Python's global `random` -- the crop and flip
draws of datas.US1K -- sees the same sequence with and without it.  `datas.US1K`, `datas.Benchmark`, train.py (`degradation:` in the
yaml) and tools/make_lr.py accept one.  The device work is one fused kernel per batch; its result is defined to the byte
(include/m2t_degrade.h) and pinned by a NumPy fp64 restatement (tests/degrade_ref.py).

Device tensors only: there is no host fallback."""
from __future__ import annotations

import math
import random
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import M2TError

CONFIG_KEYS = ("bank", "sigma", "iso_prob", "ksize", "kernels", "noise", "speckle", "gray_noise", "seed")
BENCHMARK_NOISE_ID = 1 << 63          # datas.Benchmark numbers its images from here: apart from the running counter of draw()


def default_ksize(scale: int, sigma_max: float) -> int:
    """The smallest admissible K >= 6 sigma_max + 1: K has the parity of the scale and is capped at 21 (odd) / 20 (even)."""
    top = _lib.DEGRADE_KMAX[scale]
    k = 2 - (scale & 1)
    while k < 6.0 * sigma_max + 1.0 and k < top:
        k += 2
    return k


def gaussian_kernel(K: int, sigma1: float, sigma2: float, theta: float) -> np.ndarray:
    """w[i][j] ~ exp(-(a o_j^2 + 2 b o_j o_i + c o_i^2) / 2), o_i = i - (K - 1) / 2, [[a, b], [b, c]] the inverse of
    Q(theta) diag(sigma1^2, sigma2^2) Q(theta)^T; normalised by its fp64 sum."""
    ct, st = math.cos(theta), math.sin(theta)
    v1, v2 = sigma1 * sigma1, sigma2 * sigma2
    sxx, sxy, syy = ct * ct * v1 + st * st * v2, ct * st * (v1 - v2), st * st * v1 + ct * ct * v2
    det = sxx * syy - sxy * sxy
    a, b, c = syy / det, -sxy / det, sxx / det
    o = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    oi, oj = o[:, None], o[None, :]
    w = np.exp(-0.5 * (a * oj * oj + 2.0 * b * oj * oi + c * oi * oi))
    return w / w.sum()


def _pair(name: str, v, positive: bool = False) -> Tuple[float, float]:
    try:
        lo, hi = v
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise M2TError(f"Degradation: {name} must be (lo, hi), got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi and (lo > 0.0 if positive else lo >= 0.0)):
        raise M2TError(f"Degradation: {name} must be finite with {'0 < ' if positive else '0 <= '}lo <= hi, got {v!r}")
    return lo, hi


class Degradation:
    """`Degradation(scale, bank=256, sigma=(0.2, 0.8 * scale), iso_prob=0.5, ksize=None, kernels=None, noise=(0, 8),
    speckle=(0, 0.15), gray_noise=True, seed=33)`.

    bank, sigma, iso_prob, ksize: the kernel bank -- `bank` anisotropic Gaussians of `ksize` x `ksize` taps; per kernel the draws are
        `iso = random() < iso_prob`, `sigma1 = uniform(*sigma)`, `sigma2 = sigma1 if iso else uniform(*sigma)`, `theta = uniform(0, pi)`.
    kernels: an ndarray [M, K, K] used instead (measured PSFs): K of the scale's parity, finite, every kernel summing to 1 within 1e-12.
    noise: the range of the additive level, in grey levels of the 0 .. 255 scale; speckle: the range of the multiplicative level.
    gray_noise: one variate per pixel for the three channels (ultrasound PNGs are grey replicated to RGB).
    seed: seeds the object's own `random.Random` (bank first, then the per-sample draws) and is the key of the noise generator."""

    def __init__(self, scale: int, bank: int = 256, sigma: Optional[Sequence[float]] = None, iso_prob: float = 0.5,
                 ksize: Optional[int] = None, kernels=None, noise: Sequence[float] = (0.0, 8.0), speckle: Sequence[float] = (0.0, 0.15),
                 gray_noise: bool = True, seed: int = 33):
        if scale not in (2, 3, 4):
            raise M2TError(f"Degradation: scale must be 2, 3 or 4, got {scale!r}")
        self.scale = int(scale)
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise M2TError(f"Degradation: seed must be an integer in [0, 2^64), got {seed!r}")
        self.seed = seed
        self.noise, self.speckle = _pair("noise", noise), _pair("speckle", speckle)
        self.gray_noise = bool(gray_noise)
        self._rng = random.Random(seed)
        self._noise_id = 0
        top = _lib.DEGRADE_KMAX[self.scale]
        if kernels is not None:
            k = np.asarray(kernels)
            if k.ndim != 3 or k.shape[0] < 1 or k.shape[1] != k.shape[2] or not np.issubdtype(k.dtype, np.number):
                raise M2TError(f"Degradation: kernels must be a numeric array [M, K, K], got {getattr(k, 'dtype', '')} {k.shape}")
            K = int(k.shape[1])
            if (K ^ self.scale) & 1 or not 1 <= K <= top:
                raise M2TError(f"Degradation: K = {K} is not admissible at x{self.scale} (K has the parity of the scale, at most {top})")
            k = np.ascontiguousarray(k, dtype=np.float64)
            if not np.isfinite(k).all():
                raise M2TError("Degradation: kernels holds a non-finite value")
            off = np.abs(k.reshape(k.shape[0], -1).sum(axis=1) - 1.0)
            if float(off.max()) > 1e-12:
                raise M2TError(f"Degradation: kernel {int(off.argmax())} sums to 1 {float(off.max()):+.3e}: every kernel must sum to 1 within 1e-12")
            self.sigma, self.iso_prob, self.ksize, self.kernels = None, None, K, k
        else:
            self.sigma = _pair("sigma", (0.2, 0.8 * self.scale) if sigma is None else sigma, positive=True)
            self.iso_prob = float(iso_prob)
            if not 0.0 <= self.iso_prob <= 1.0:
                raise M2TError(f"Degradation: iso_prob must be in [0, 1], got {iso_prob!r}")
            if isinstance(bank, bool) or not isinstance(bank, int) or bank < 1:
                raise M2TError(f"Degradation: bank must be an integer >= 1, got {bank!r}")
            K = default_ksize(self.scale, self.sigma[1]) if ksize is None else ksize
            if isinstance(K, bool) or not isinstance(K, int) or (K ^ self.scale) & 1 or not 1 <= K <= top:
                raise M2TError(f"Degradation: ksize = {K!r} is not admissible at x{self.scale} (the parity of the scale, at most {top})")
            self.ksize = K
            rows = []
            for _ in range(bank):
                iso = self._rng.random() < self.iso_prob
                s1 = self._rng.uniform(*self.sigma)
                s2 = s1 if iso else self._rng.uniform(*self.sigma)
                theta = self._rng.uniform(0.0, math.pi)
                rows.append(gaussian_kernel(K, s1, s2, theta))
            self.kernels = np.stack(rows)
        self._dev = {}

    def __len__(self) -> int:
        return int(self.kernels.shape[0])

    # -------------------------------------------------------------------------------------------------------------- draws
    def draw_levels(self, rng) -> Tuple[int, float, float]:
        """(bank index, sigma_add, sigma_speckle) from `rng`: randrange(M), uniform(*noise), uniform(*speckle)."""
        index = rng.randrange(len(self))
        return index, rng.uniform(*self.noise), rng.uniform(*self.speckle)

    def draw(self) -> Tuple[int, float, float, int]:
        """(bank index, sigma_add, sigma_speckle, noise_id) from the object's own generator; noise_id is a running 64-bit counter."""
        index, sa, ss = self.draw_levels(self._rng)
        nid = self._noise_id
        self._noise_id = (nid + 1) & ((1 << 64) - 1)
        return index, sa, ss, nid

    def get_state(self) -> dict:
        """Plain picklable data: where the per-sample draws stand (the bank is a function of the constructor's arguments)."""
        return {"random": self._rng.getstate(), "noise_id": self._noise_id}

    def set_state(self, state: dict) -> None:
        r = state["random"]
        self._rng.setstate((r[0], tuple(r[1]), r[2]))
        self._noise_id = int(state["noise_id"])

    def __deepcopy__(self, memo):
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new._rng = random.Random()
        new._rng.setstate(self._rng.getstate())
        new._dev = {}
        return new

    # -------------------------------------------------------------------------------------------------------------- device
    def bank_on(self, device):
        """The bank as a float64 [M, K, K] tensor on `device`, uploaded on first use and kept."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise M2TError("Degradation keeps its bank on the device: a HIP device is required")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.kernels).to(device)
        return self._dev[device]

    @property
    def bank(self):
        return self.bank_on("cuda")

    def apply_image(self, hr_u8_dev, index: int = 0, sigma_add: float = 0.0, sigma_speckle: float = 0.0, noise_id: int = 0, out=None):
        """uint8 [H, W, 3] on the device -> the degraded uint8 [H // s, W // s, 3] (m2t_degrade_image_u8), kernel `index` of the bank."""
        import torch
        t = hr_u8_dev
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_cuda:
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise M2TError(f"apply_image: a uint8 [H,W,3] device tensor is required, got {got}")
        t = t.contiguous()
        H, W = int(t.shape[0]), int(t.shape[1])
        s = self.scale
        if H < s or W < s:
            raise M2TError(f"apply_image: image {H}x{W} is smaller than one LR pixel at x{s}")
        if out is None:
            out = torch.empty(H // s, W // s, 3, dtype=torch.uint8, device=t.device)
        elif out.dtype != torch.uint8 or out.numel() != (H // s) * (W // s) * 3 or out.device != t.device or not out.is_contiguous():
            raise M2TError(f"apply_image: out must be a contiguous uint8 tensor of {(H // s) * (W // s) * 3} elements on {t.device}")
        bank = self.bank_on(t.device)
        with torch.cuda.device(t.device):
            _lib.check(_lib.load().m2t_degrade_image_u8(_lib.ptr(t), H, W, 3, _lib.ptr(bank), len(self), self.ksize, int(index), s,
                                                        self.seed, int(noise_id) & ((1 << 64) - 1), float(sigma_add), float(sigma_speckle),
                                                        int(self.gray_noise), _lib.ptr(out), _lib.stream_ptr()), "m2t_degrade_image_u8")
        return out


def from_config(scale: int, cfg) -> Optional[Degradation]:
    """The yaml mapping `degradation:` of train.py -> a Degradation (None stays None).  `kernels` may name an .npy file."""
    if cfg is None:
        return None
    kw = check_config(cfg)
    if isinstance(kw.get("kernels"), str):
        kw["kernels"] = np.load(kw["kernels"])
    for k in ("sigma", "noise", "speckle"):
        if isinstance(kw.get(k), list):
            kw[k] = tuple(kw[k])
    return Degradation(int(scale), **kw)


def check_config(cfg) -> dict:
    """A copy of the mapping; an unknown sub-key is an M2TError that names it."""
    if not isinstance(cfg, dict):
        raise M2TError(f"degradation must be a mapping of Degradation's arguments, got {type(cfg).__name__}")
    unknown = sorted(str(k) for k in cfg if k not in CONFIG_KEYS)
    if unknown:
        raise M2TError(f"unknown degradation key{'s' if len(unknown) > 1 else ''}: {', '.join(unknown)} (known: {', '.join(CONFIG_KEYS)})")
    return dict(cfg)
