"""LR synthesis beyond bicubic (include/m2t_degrade.h, k_degrade.hip): the classical degradation model
`LR = ((HR (*) k) downsampled by s) * (1 + n_s) + n_a` with the blur kernel `k` and the two noise levels drawn per sample.

The reference trains on MATLAB-bicubic pairs only and carries its noise augmentation as dead code (datas/us1k.py:156-167).  A
`Degradation` holds a bank of anisotropic Gaussian kernels (or measured PSFs handed in as an array), built on the host in fp64 and
uploaded once, and a `random.Random` of its own for the per-sample draws, so that Python's global `random` -- the crop and flip
draws of datas.US1K -- sees the same sequence with and without it.  `datas.US1K`, `datas.Benchmark`, train.py (`degradation:` in the
yaml) and tools/make_lr.py accept one.  The device work is one fused kernel per batch; its result is defined to the byte
(include/m2t_degrade.h) and pinned by a NumPy fp64 restatement (tests/degrade_ref.py).

`jpeg=(lo, hi)` ends the pipeline with a simulated baseline JPEG round trip of a per-sample quality (include/m2t_jpeg.h, k_jpeg.hip; NumPy
restatement tests/jpeg_ref.py); `jpeg_roundtrip` applies the stage alone to a uint8 image.

Device tensors only: there is no host fallback."""
from __future__ import annotations

import math
import random
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import M2TError

CONFIG_KEYS = ("bank", "sigma", "iso_prob", "ksize", "kernels", "noise", "speckle", "gray_noise", "seed", "jpeg", "jpeg_prob")
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


def jpeg_constants() -> np.ndarray:
    """The 320 fp64 constants of include/m2t_jpeg.h: T[u][x] = c_u cos((2x + 1) u pi / 16) row-major, then recip[k] = 1.0 / k
    (recip[0] = 0, unused).  T is evaluated in 50-digit decimal arithmetic -- cos(pi / 16) by two half-angle steps from cos(pi / 4),
    its multiples by the Chebyshev recurrence -- and rounded once, so every entry is the correctly rounded value."""
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        one, two = decimal.Decimal(1), decimal.Decimal(2)
        c = two.sqrt() / two                                  # cos(pi / 4)
        for _ in range(2):
            c = ((one + c) / two).sqrt()                      # cos(pi / 8), cos(pi / 16)
        cos = [one, c]
        for _ in range(30):
            cos.append(two * c * cos[-1] - cos[-2])           # cos(k pi / 16), k = 0 .. 31
        c0 = (one / decimal.Decimal(8)).sqrt()
        T = [float((c0 if u == 0 else one / two) * cos[(2 * x + 1) * u % 32]) for u in range(8) for x in range(8)]
    recip = [0.0] + [1.0 / k for k in range(1, 256)]
    return np.array(T + recip, dtype=np.float64)


_JPEG_CONSTS = None
_JPEG_DEV = {}


def _jpeg_constants_on(device):
    """The constants as a float64 [320] tensor on `device`, uploaded on first use and kept (one per process and device)."""
    import torch
    global _JPEG_CONSTS
    device = torch.device(device)
    if device.type != "cuda":
        raise M2TError("the JPEG stage runs on the device: a HIP device is required")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _JPEG_DEV:
        if _JPEG_CONSTS is None:
            _JPEG_CONSTS = jpeg_constants()
        _JPEG_DEV[device] = torch.from_numpy(_JPEG_CONSTS).to(device)
    return _JPEG_DEV[device]


def jpeg_roundtrip(img_u8_dev, quality: int, out=None):
    """uint8 [H, W, 3] on the device -> the image after a simulated baseline JPEG round trip at 4:4:4 (m2t_jpeg_image_u8,
    include/m2t_jpeg.h), `quality` 1 .. 100; the 8 x 8 blocks start at the image's origin."""
    import torch
    t = img_u8_dev
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_cuda:
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise M2TError(f"jpeg_roundtrip: a uint8 [H,W,3] device tensor is required, got {got}")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise M2TError(f"jpeg_roundtrip: quality must be an integer 1 .. 100, got {quality!r}")
    t = t.contiguous()
    H, W = int(t.shape[0]), int(t.shape[1])
    if H < 1 or W < 1:
        raise M2TError(f"jpeg_roundtrip: the image {H}x{W} is empty")
    if out is None:
        out = torch.empty_like(t)
    elif out.dtype != torch.uint8 or out.numel() != t.numel() or out.device != t.device or not out.is_contiguous() or out.data_ptr() == t.data_ptr():
        raise M2TError(f"jpeg_roundtrip: out must be another contiguous uint8 tensor of {t.numel()} elements on {t.device}")
    consts = _jpeg_constants_on(t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().m2t_jpeg_image_u8(_lib.ptr(t), H, W, 3, _lib.ptr(consts), quality, _lib.ptr(out), _lib.stream_ptr()),
                   "m2t_jpeg_image_u8")
    return out


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
    speckle=(0, 0.15), gray_noise=True, seed=33, jpeg=None, jpeg_prob=1.0)`.

    bank, sigma, iso_prob, ksize: the kernel bank -- `bank` anisotropic Gaussians of `ksize` x `ksize` taps; per kernel the draws are
        `iso = random() < iso_prob`, `sigma1 = uniform(*sigma)`, `sigma2 = sigma1 if iso else uniform(*sigma)`, `theta = uniform(0, pi)`.
    kernels: an ndarray [M, K, K] used instead (measured PSFs): K of the scale's parity, finite, every kernel summing to 1 within 1e-12.
    noise: the range of the additive level, in grey levels of the 0 .. 255 scale; speckle: the range of the multiplicative level.
    gray_noise: one variate per pixel for the three channels (ultrasound PNGs are grey replicated to RGB).
    seed: seeds the object's own `random.Random` (bank first, then the per-sample draws) and is the key of the noise generator.
    jpeg, jpeg_prob: `jpeg=(lo, hi)`, integer qualities with 1 <= lo <= hi <= 100, ends the pipeline with a simulated baseline JPEG round
        trip (include/m2t_jpeg.h) of a quality drawn per sample by `draw_jpeg()`; with probability 1 - jpeg_prob a sample skips the
        stage.  None: no stage, and not one draw, call or allocation more than without the argument."""

    def __init__(self, scale: int, bank: int = 256, sigma: Optional[Sequence[float]] = None, iso_prob: float = 0.5,
                 ksize: Optional[int] = None, kernels=None, noise: Sequence[float] = (0.0, 8.0), speckle: Sequence[float] = (0.0, 0.15),
                 gray_noise: bool = True, seed: int = 33, jpeg: Optional[Sequence[int]] = None, jpeg_prob: float = 1.0):
        if scale not in (2, 3, 4):
            raise M2TError(f"Degradation: scale must be 2, 3 or 4, got {scale!r}")
        self.scale = int(scale)
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise M2TError(f"Degradation: seed must be an integer in [0, 2^64), got {seed!r}")
        self.seed = seed
        self.noise, self.speckle = _pair("noise", noise), _pair("speckle", speckle)
        self.gray_noise = bool(gray_noise)
        if jpeg is not None:
            try:
                lo, hi = jpeg
            except (TypeError, ValueError):
                raise M2TError(f"Degradation: jpeg must be None or (lo, hi), got {jpeg!r}") from None
            if any(isinstance(v, bool) or not isinstance(v, int) for v in (lo, hi)) or not 1 <= lo <= hi <= 100:
                raise M2TError(f"Degradation: jpeg must be integer qualities with 1 <= lo <= hi <= 100, got {jpeg!r}")
            jpeg = (lo, hi)
        self.jpeg = jpeg
        if isinstance(jpeg_prob, bool) or not isinstance(jpeg_prob, (int, float)) or not 0.0 <= jpeg_prob <= 1.0:
            raise M2TError(f"Degradation: jpeg_prob must be a number in [0, 1], got {jpeg_prob!r}")
        self.jpeg_prob = float(jpeg_prob)
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

    def draw_jpeg(self, rng=None) -> int:
        """The quality of the next sample from `rng` (the object's own generator by default): two draws, always --
        `apply = random() < jpeg_prob`, `q = randint(lo, hi)` -- and `q if apply else 0` (0: the stage is skipped)."""
        if self.jpeg is None:
            raise M2TError("Degradation: draw_jpeg() needs jpeg=(lo, hi)")
        rng = self._rng if rng is None else rng
        apply = rng.random() < self.jpeg_prob
        q = rng.randint(*self.jpeg)
        return q if apply else 0

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

    def jpeg_constants_on(self, device):
        """The constants of the JPEG stage (T and recip, include/m2t_jpeg.h) as a float64 [320] tensor on `device`, uploaded once."""
        return _jpeg_constants_on(device)

    @property
    def bank(self):
        return self.bank_on("cuda")

    def apply_image(self, hr_u8_dev, index: int = 0, sigma_add: float = 0.0, sigma_speckle: float = 0.0, noise_id: int = 0, out=None,
                    quality: int = 0):
        """uint8 [H, W, 3] on the device -> the degraded uint8 [H // s, W // s, 3] (m2t_degrade_image_u8), kernel `index` of the bank.
        `quality` 1 .. 100 ends with the JPEG stage (m2t_degrade_jpeg_image_u8); 0 is the call without it."""
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
        if isinstance(quality, bool) or not isinstance(quality, int):
            raise M2TError(f"apply_image: quality must be an integer 0 .. 100, got {quality!r}")
        if quality != 0:
            consts = _jpeg_constants_on(t.device)
            with torch.cuda.device(t.device):
                _lib.check(_lib.load().m2t_degrade_jpeg_image_u8(_lib.ptr(t), H, W, 3, _lib.ptr(bank), len(self), self.ksize, int(index), s,
                                                                 self.seed, int(noise_id) & ((1 << 64) - 1), float(sigma_add),
                                                                 float(sigma_speckle), int(self.gray_noise), _lib.ptr(consts), quality,
                                                                 _lib.ptr(out), _lib.stream_ptr()), "m2t_degrade_jpeg_image_u8")
            return out
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
    for k in ("sigma", "noise", "speckle", "jpeg"):
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
