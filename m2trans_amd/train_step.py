"""The training step of the reference (train.py:173-214, setup :76-82,358), driven on MI355X.

``TrainStep`` restates the hot loop body

    optimizer.zero_grad(); sr = model(lr); loss = L1Loss()(sr, hr) * lambda_l1 (+ const clip term);
    loss.backward(); optimizer.step()

as five C-ABI calls on one stream (forward, loss+seed, backward, fused Adam; plus the RCCL
all-reduce of the flat gradient buffer when world_size > 1 -- in two contiguous pieces, the first of
which (tail + 3/4 of the body) starts as soon as m2t_backward has finished it, on a communication
stream that runs under the rest of the backward pass), with no host synchronisation:
the loss stays on the device (the reference's three ``float(loss)`` syncs per step,
train.py:212-214, are left to the caller's logging cadence).

Data parallelism (replaces nn.DataParallel, train.py:73): one process per GPU, persistent
replicas, equal shards of the global batch; each rank divides its L1 sum by the GLOBAL element
count, so SUM-all-reduced gradients equal the full-batch gradient.

Gradient accumulation (``accum_steps=k``; replaces torch's AccumulateGrad under several ``loss.backward()`` calls before one
``optimizer.step()``): a micro-batch is a rank that runs later on the same device -- the same global divisor, the sum taken by
one streaming HIP pass per micro-batch (m2t_grad_accumulate), one exchange and one Adam pass per k micro-batches.

Optimizer options (all off by default; replace ``clip_grad_norm_``, Adam's ``weight_decay`` / ``decoupled_weight_decay`` -- the
knob train.py:81 passes -- and a hand-kept EMA copy): the global norm of the accumulated, all-reduced gradient goes into a
device-resident record (m2t_grad_norm: two launches, fp64, no atomics), and ONE pass (m2t_adam_step_ex) clips, decays, steps
and updates the EMA weights -- or, with ``skip_nonfinite`` and a non-finite norm, touches nothing.  No host synchronisation.

Pixel losses (``pixel_loss=``; the criteria the reference offers next to L1, losses.py:225-230 l1 / sl1 / l2 and :287-297
L1_Charbonnier_loss): the kind only selects the per-pixel function inside the kernel that takes the loss (m2t_pixel_loss /
m2t_pixel_loss_deferred), so every kind runs the schedule of the L1 step -- the seed fused into the x4 tail backward, accumulation,
the overlapped exchange and the optimizer options included.

Optional loss terms (all off by default; LOSS_TERMS below is their one table, and its order -- SSIM, MS-SSIM, FFT, VIF, GMSD, wavelet,
consistency, then the perceptual term, which has a path of its own behind the table -- is the order of the calls).  Every term that is on takes the MATERIALISED seed: the immediate pixel loss, then one
``m2t_<term>_loss`` call per term that adds its gradient into the seed, then the backward pass; the seed fused into the x4 tail
backward does not apply.  An SR size a term does not take is refused on the host before anything is launched.  With a weight of 0
nothing is allocated for the term and the step issues the calls it issued before.  Value and gradient are HIP, fp64 inside unless
said otherwise.

* ``lambda_ssim`` (the reference imports SSIMLoss from piq next to the pixel criteria, losses.py:8, and scores every epoch by SSIM,
  utils.py:232-234): ``lambda_ssim * (1 - mean SSIM)`` per RGB channel in the pytorch_msssim.ssim / piq.ssim(downsample=False) form --
  piq.SSIMLoss's default ``downsample=True`` pooling is NOT applied (m2t_ssim_loss; SR height and width >= 11).
* ``lambda_msssim`` (MultiScaleSSIMLoss of the same import; L1 + MS-SSIM is the recipe of Zhao et al.): ``lambda_msssim * (1 - mean
  MS-SSIM)`` per image and RGB channel in the pytorch_msssim.ms_ssim / piq.multi_scale_ssim form, five levels with the 2 x 2 average
  between them (m2t_msssim_loss of include/m2t_msssim.h; SR height and width > 160).  An (image, channel) with a non-positive level
  mean has MS-SSIM 0 and adds no gradient.
* ``lambda_fft``, ``fft_norm`` (the reference imports torch.fft in losses.py:5 and never calls it -- the term is MIMO-UNet's L1 on the
  Fourier coefficients): ``lambda_fft * mean(|Re D|, |Im D|)`` with ``D = rfft2(clamp(sr) / R - hr / R, norm=fft_norm)`` per RGB
  channel (m2t_fft_loss of include/m2t_spectral.h: a mixed-radix Stockham FFT in LDS, fp32 butterflies; SR height and width even,
  8 .. 2048, of the form 2^a 3^b).
* ``lambda_vif`` (VIFLoss of the same import): ``lambda_vif * (1 - mean VIF)`` per image, the pixel-domain VIF of Sheikh & Bovik in
  the piq.vif_p form on the luminance of ``clamp(sr, 0, rgb_range)`` and ``hr``, four scales, windows of 17 / 9 / 5 / 3 taps,
  sigma_n_sq = 2 (m2t_vif_loss of include/m2t_vif.h; SR height and width >= 41).  VIF exceeds 1 for a contrast-enhanced output, so
  the term may be negative; it is not clipped.
* ``lambda_gmsd`` (piq ships GMSDLoss next to those classes; the reference reports GMSD for every model, test.py:95-122):
  ``lambda_gmsd * mean GMSD`` per image, the deviation of the gradient-magnitude similarity map of the pooled luminance of
  ``clamp(sr, 0, rgb_range)`` and ``hr`` (m2t_gmsd_loss of include/m2t_gmsd.h; SR height and width >= 2).  A distortion: there is no
  "1 -".  Exactly 0 gradient where the pooled output is locally flat (torch's autograd gives NaN there).
* ``lambda_wavelet``, ``wavelet=``, ``wavelet_levels=``, ``wavelet_band_weights=``, ``wavelet_eps=`` (the model itself moves between
  its scales through a Haar DWT): ``lambda_wavelet * mean`` over the coefficients of ``sum_band w_band rho(c_band)`` on the undecimated
  (stationary) wavelet transform of ``clamp(sr, 0, rgb_range) / rgb_range - hr / rgb_range`` with periodic borders: ``'haar'``, ``'db2'``
  or a pair of tap lists, 1 .. 3 levels, by default an L1 on every detail band and nothing on LL (m2t_wavelet_loss of
  include/m2t_wavelet.h; SR height and width >= (taps - 1) * 2^(levels - 1) + 1).
* ``lambda_consistency``, ``consistency_eps`` (the "dual regression" / cycle term; the only one that compares with the LR input and
  not with HR): ``lambda_consistency * mean rho((D(clamp(sr, 0, rgb_range)) - lr) / rgb_range)`` over the LR elements, D the bicubic
  down-sampler that made the training pairs, rho = |.| or Charbonnier with ``consistency_eps`` (m2t_consistency_loss of
  include/m2t_consistency.h).  Its target is the step's own ``lr_img``, which also sizes its scratch: the last row of the table.
* ``lambda_perceptual``, ``perceptual_loss=`` (PerceptualLoss of the reference's losses.py:222-270): ``lambda_perceptual * sum_k w_k
  mean(crit(F_k(sr) - F_k(hr)))`` on VGG19 features; the tower, its weights, its workspace, the criterion and the tap weights are
  those of the losses.PerceptualLoss object (m2t_vgg_loss of include/m2t_perceptual.h, bf16 compute; SR height and width >= 16).

Parameter groups and frozen tensors (``param_groups=``; replaces ``torch.optim.Adam([{"params": ..., "lr": ...,
"weight_decay": ...}, ...])`` over a model part of which has ``requires_grad = False``; param_groups.py resolves the spec by name):
a group has its own ``lr_scale`` and ``weight_decay`` and may be ``frozen``.  The flat buffer is described by a segment table that
is uploaded ONCE at construction; each step hands the groups' values over by value: m2t_grad_norm_groups (the norm over the
trainable elements) and ONE m2t_adam_step_groups pass (include/m2t_groups.h), which neither read nor write a frozen element.  When
a whole stage (head / body.b / tail) is frozen, every route of forward_backward calls m2t_backward_ex with the stage flags instead
of m2t_backward.  ``param_groups="requires_grad"`` freezes the trainable tensors whose ``requires_grad`` is False.  With
``param_groups=None`` (the default) nothing is allocated and the step issues the calls it issued before.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib
from .dist import GradBucket, global_divisor
from .M2Trans_network import M2Trans
from .param_groups import resolve_param_groups


def cosine_lr(epoch: int, lr0: float = 1e-4, eta_min: float = 1e-6, t_max: float = 200.0) -> float:
    """CosineAnnealingLR(optimizer, float(epochs), eta_min) evaluated at `epoch` scheduler steps
    (train.py:82,358; the scheduler is stepped once per epoch)."""
    return eta_min + 0.5 * (lr0 - eta_min) * (1.0 + math.cos(math.pi * epoch / t_max))


# pixel_loss name -> (kind of include/m2t.h's m2t_pixel_loss_kind, canonical name, name of its parameter, default)
PIXEL_LOSSES = {"l1": (0, "l1", None, None), "mse": (1, "mse", None, None), "l2": (1, "mse", None, None),
                "charbonnier": (2, "charbonnier", "eps", 1e-6),                  # losses.py:295: sqrt(diff * diff + 1e-6)
                "smooth_l1": (3, "smooth_l1", "beta", 1.0), "sl1": (3, "smooth_l1", "beta", 1.0)}      # nn.SmoothL1Loss's default


def resolve_pixel_loss(name, param=None):
    """(kind, canonical name, parameter) of TrainStep's ``pixel_loss`` / ``pixel_loss_param``; M2TError for an unknown name, a
    parameter given to a kind that takes none, or an eps / beta that is not a finite number > 0.  The parameter of a kind that
    takes none is None."""
    key = name.lower() if isinstance(name, str) else name
    if not isinstance(key, str) or key not in PIXEL_LOSSES:
        raise _lib.M2TError(f"pixel_loss must be one of {sorted(PIXEL_LOSSES)}, got {name!r}")
    kind, canon, pname, default = PIXEL_LOSSES[key]
    if pname is None:
        if param is not None:
            raise _lib.M2TError(f"pixel_loss {canon!r} takes no parameter, got pixel_loss_param={param!r}")
        return kind, canon, None
    if param is None:
        param = default
    try:
        value = float(param)
    except (TypeError, ValueError):
        raise _lib.M2TError(f"pixel_loss {canon!r}: {pname} must be a finite number > 0, got {param!r}") from None
    # (the library takes the parameter as a float: what rounds to 0 or inf there is refused here, at construction)
    as_f32 = C.c_float(value).value
    if not (math.isfinite(as_f32) and as_f32 > 0.0):
        hint = " (beta = 0 is the l1 loss: use pixel_loss='l1')" if canon == "smooth_l1" and value == 0.0 else ""
        raise _lib.M2TError(f"pixel_loss {canon!r}: {pname} must be a finite number > 0, got {param!r}{hint}")
    return kind, canon, value


def resolve_lambda(name: str, value) -> float:
    """TrainStep's ``lambda_<name>`` as a float; M2TError unless it is a finite number >= 0."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and v >= 0.0):
        raise _lib.M2TError(f"lambda_{name} must be a finite number >= 0, got {value!r}")
    return v


resolve_lambda_ssim = functools.partial(resolve_lambda, "ssim")
resolve_lambda_msssim = functools.partial(resolve_lambda, "msssim")
resolve_lambda_fft = functools.partial(resolve_lambda, "fft")
resolve_lambda_vif = functools.partial(resolve_lambda, "vif")
resolve_lambda_gmsd = functools.partial(resolve_lambda, "gmsd")
resolve_lambda_wavelet = functools.partial(resolve_lambda, "wavelet")
resolve_lambda_perceptual = functools.partial(resolve_lambda, "perceptual")
resolve_lambda_consistency = functools.partial(resolve_lambda, "consistency")


def resolve_consistency_eps(value) -> float:
    """TrainStep's ``consistency_eps`` as a float; M2TError unless it is a finite number >= 0 (0 = L1, > 0 = Charbonnier)."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and v >= 0.0):
        raise _lib.M2TError(f"consistency_eps must be a finite number >= 0, got {value!r}")
    return v

_S3 = math.sqrt(3.0)
_DB2 = ((1.0 + _S3) / 8.0, (3.0 + _S3) / 8.0, (3.0 - _S3) / 8.0, (1.0 - _S3) / 8.0)
# the built-in analysis pairs of include/m2t_wavelet.h: the orthonormal filters divided by sqrt(2) (sum lo = 1, sum hi = 0)
WAVELETS = {
    "haar": ((0.5, 0.5), (0.5, -0.5)),
    "db2": (_DB2, tuple((-1.0) ** k * _DB2[3 - k] for k in range(4))),
}


class Wavelet(NamedTuple):
    """What ``resolve_wavelet`` gives: ``wavelet`` as it is kept and written to a checkpoint (a name, or the two tap lists), the
    taps, the level count, the band weights (None = 1 for every detail band, 0 for LL) and eps."""
    wavelet: object
    lo: tuple
    hi: tuple
    levels: int
    band_weights: Optional[tuple]
    eps: float


def resolve_wavelet(wavelet="haar", levels=2, band_weights=None, eps=0.0) -> Wavelet:
    """The wavelet arguments of TrainStep / losses.wavelet_loss / losses.swt2, by the rules of include/m2t_wavelet.h; M2TError
    naming what is wrong: the name, the tap lists, the level count, the weight vector or eps."""
    if isinstance(wavelet, str):
        key = wavelet.lower()
        if key not in WAVELETS:
            raise _lib.M2TError(f"wavelet must be one of {sorted(WAVELETS)} or a pair (lo, hi) of tap lists, got {wavelet!r}")
        canon, (lo, hi) = key, WAVELETS[key]
    else:
        try:
            lo, hi = (tuple(float(v) for v in f) for f in wavelet)
        except (TypeError, ValueError):
            raise _lib.M2TError(f"wavelet must be one of {sorted(WAVELETS)} or a pair (lo, hi) of tap lists, got {wavelet!r}") from None
        if len(lo) != len(hi) or not 2 <= len(lo) <= _lib.WAVELET_MAX_TAPS or not all(math.isfinite(v) for v in lo + hi):
            raise _lib.M2TError(f"wavelet taps: lo and hi must be two lists of equal length, 2 to {_lib.WAVELET_MAX_TAPS} finite numbers "
                                f"each, got {wavelet!r}")
        canon = (list(lo), list(hi))
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= _lib.WAVELET_MAX_LEVELS:
        raise _lib.M2TError(f"wavelet_levels must be an integer from 1 to {_lib.WAVELET_MAX_LEVELS}, got {levels!r}")
    if band_weights is not None:
        try:
            band_weights = tuple(float(v) for v in band_weights)
        except (TypeError, ValueError):
            band_weights = ()
        if len(band_weights) != 3 * levels + 1 or not all(math.isfinite(v) and v >= 0.0 for v in band_weights) or not any(band_weights):
            raise _lib.M2TError(f"wavelet_band_weights must be {3 * levels + 1} finite numbers >= 0, not all 0 (three detail bands per level, "
                                f"then LL), got {band_weights!r}")
    try:
        e = float(eps)
    except (TypeError, ValueError):
        e = math.nan
    if not (math.isfinite(e) and e >= 0.0):
        raise _lib.M2TError(f"wavelet_eps must be a finite number >= 0, got {eps!r}")
    return Wavelet(canon, lo, hi, levels, band_weights, e)


def wavelet_call_args(w: Wavelet) -> tuple:
    """The wavelet arguments of the C entries (lo, hi, taps, levels, band_weights, eps): host double arrays, None for the default
    weights."""
    arr = lambda v: (C.c_double * len(v))(*v)
    return arr(w.lo), arr(w.hi), len(w.lo), w.levels, None if w.band_weights is None else arr(w.band_weights), w.eps


def resolve_fft_norm(name) -> str:
    """TrainStep's ``fft_norm``: 'backward' (torch.fft's default, no scaling) or 'ortho' (1 / sqrt(H W)); M2TError otherwise."""
    key = name.lower() if isinstance(name, str) else name
    if not isinstance(key, str) or key not in _lib.FFT_NORMS:
        raise _lib.M2TError(f"fft_norm must be one of {sorted(_lib.FFT_NORMS)}, got {name!r}")
    return key


def msssim_size_supported(h: int, w: int) -> bool:
    """The sizes the multi-scale term takes (the rule of include/m2t_msssim.h, decided on the host): min(H, W) > 160."""
    return min(int(h), int(w)) >= _lib.MSSSIM_MIN_SIDE


def vif_size_supported(h: int, w: int) -> bool:
    """The sizes the information-fidelity term takes (the rule of include/m2t_vif.h, decided on the host): min(H, W) >= 41."""
    return min(int(h), int(w)) >= _lib.VIF_MIN_SIDE


def gmsd_size_supported(h: int, w: int) -> bool:
    """The sizes the GMSD term takes (the rule of include/m2t_gmsd.h, decided on the host): min(H, W) >= 2."""
    return min(int(h), int(w)) >= _lib.GMSD_MIN_SIDE


def wavelet_size_supported(h: int, w: int, levels: int = 1, taps: int = 2) -> bool:
    """The sizes the wavelet term takes (the rule of include/m2t_wavelet.h, decided on the host): min(H, W) >= (taps - 1) *
    2^(levels - 1) + 1."""
    return min(int(h), int(w)) >= _lib.wavelet_min_side(taps, levels)


def perceptual_size_supported(h: int, w: int) -> bool:
    """The sizes the VGG19 feature term takes (the rule of include/m2t_perceptual.h, decided on the host): min(H, W) >= 16."""
    return min(int(h), int(w)) >= _lib.VGG_MIN_SIDE


FFT_SIZE_RULE = "even, 8 .. 2048 and of the form 2^a * 3^b"


def fft_size_supported(n: int) -> bool:
    """The sizes the HIP transform takes along one axis (the rule of include/m2t_spectral.h, decided on the host)."""
    n = int(n)
    if n < 8 or n > 2048 or n % 2:
        return False
    while n % 2 == 0:
        n //= 2
    while n % 3 == 0:
        n //= 3
    return n == 1


class LossTerm(NamedTuple):
    """One optional term whose scratch the step owns.  From the name follow the step's attributes ``lambda_<n>`` (weight, 0 = off),
    ``<n>_loss`` (device float [1], already weighted: this rank's share of the global mean) and ``_<n>_scratch`` ((B, H, W) of the
    target -> the kernels' scratch, allocated once per plan shape), and the entries ``m2t_<n>_loss`` / ``m2t_<n>_loss_scratch_bytes``;
    the fields are what differs between the terms.  The two refusals follow "lambda_<n> > 0: " and are formatted with B, Hs, Ws of the
    target (and, by position, with scratch_tail)."""
    name: str
    size_ok: Callable       # (Hs, Ws) -> bool: the target sizes the kernels take, decided on the host
    too_small: str          # the refusal of a size outside that rule
    no_scratch: str         # the refusal of a shape the library names no scratch size for
    count: Callable         # (B, Hs, Ws) -> what the term's mean runs over on this rank (the global divisor is built from it)
    extra: Callable         # (step) -> the term's own arguments of m2t_<n>_loss, between rgb_range and the value
    shape_args: Callable = lambda step: ()      # (step) -> what size_ok and m2t_<n>_loss_scratch_bytes take behind the sizes
    target: str = "hr_img"                      # the image of the (micro-)batch the term holds SR against: it sizes count and scratch
    scratch_entry: Optional[str] = None         # the scratch size entry, where it is not m2t_<n>_loss_scratch_bytes
    scratch_tail: Callable = lambda step: ()    # (step) -> that entry's trailing arguments that are no part of the shape


# in call order: pixel -> these (each if on) -> the perceptual term (if on) -> backward
LOSS_TERMS = (
    LossTerm("ssim", lambda hs, ws: min(hs, ws) >= 11,
             "the SR image {Hs}x{Ws} is smaller than the 11 x 11 SSIM window",
             "the SR image {Hs}x{Ws} is smaller than the 11 x 11 SSIM window",
             lambda b, hs, ws: b * 3 * (hs - 10) * (ws - 10),         # entries of the valid map
             lambda step: ()),
    LossTerm("msssim", msssim_size_supported,
             "the SR image {Hs}x{Ws} is too small for five levels under the 11-tap window (height and width must be larger than 160)",
             "no scratch size for a batch of {B} SR images {Hs}x{Ws} (B * 3 <= 65535)",
             lambda b, hs, ws: b * 3,                                 # (image, channel) pairs
             lambda step: ()),
    LossTerm("fft", lambda hs, ws: fft_size_supported(hs) and fft_size_supported(ws),
             "the SR image {Hs}x{Ws} is not supported by the HIP transform (height and width must be " + FFT_SIZE_RULE + ")",
             "no scratch size for a batch of {B} SR images {Hs}x{Ws} (B * 3 <= 65535; height and width " + FFT_SIZE_RULE + ")",
             lambda b, hs, ws: b * 3 * hs * (ws // 2 + 1) * 2,        # reals of the half spectrum
             lambda step: (_lib.FFT_NORMS[step.fft_norm],)),
    LossTerm("vif", vif_size_supported,
             "the SR image {Hs}x{Ws} is too small for four scales under the 17 / 9 / 5 / 3-tap windows (height and width must be at "
             "least 41)",
             "no scratch size for a batch of {B} SR images {Hs}x{Ws} (B <= 65535)",
             lambda b, hs, ws: b,                                     # images (luminance: not times 3)
             lambda step: (_lib.VIF_SIGMA_N_SQ,)),
    LossTerm("gmsd", gmsd_size_supported,
             "the SR image {Hs}x{Ws} is smaller than one 2 x 2 cell (height and width must be at least 2)",
             "no scratch size for a batch of {B} SR images {Hs}x{Ws} (B <= 65535)",
             lambda b, hs, ws: b,                                     # images (luminance: not times 3)
             lambda step: ()),
    LossTerm("wavelet", wavelet_size_supported,
             "the SR image {Hs}x{Ws} is smaller than the reach of the filters (height and width must be at least (taps - 1) * "
             "2^(levels - 1) + 1)",
             "no scratch size for a batch of {B} SR images {Hs}x{Ws} (B * 3 <= 65535)",
             lambda b, hs, ws: b * 3 * hs * ws,                       # coefficients of one band
             lambda step: step._wavelet_args(),
             lambda step: step._wavelet_shape_args()),
    # the one term held against the LR input: every LR size is taken, the library alone decides whether it names a scratch size
    LossTerm("consistency", lambda h0, w0: True, "",
             "no scratch size for a batch of {B} LR images {Hs}x{Ws} at scale {0} (B * 3 <= 65535, SR sides at most 16384)",
             lambda b, h0, w0: b * 3 * h0 * w0,                       # LR elements
             lambda step: (float(step.consistency_eps),),
             target="lr_img", scratch_entry="m2t_consistency_scratch_bytes", scratch_tail=lambda step: (int(step.model.scale),)),
)
_TERM = {t.name: t for t in LOSS_TERMS}


_STREAMS: dict = {}


def _shared_stream(device, role: str):
    """One extra stream per (device, role) for the whole process.  Every HIP stream takes one of the runtime's few hardware queues
    (4 by default); a process that builds several TrainStep objects one after the other (bench.py's `also` workloads) would otherwise
    leave a trail of streams behind, and a later plan's main and side stream can end up on the same queue (measured: -10 ... -40 %)."""
    key = (str(torch.device(device)), role)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=device)
    return _STREAMS[key]


def _refuse_mid_cycle(step, what: str):
    """A setting that changes what a micro-batch computes may not change between the micro-batches of one optimizer step."""
    if getattr(step, "micro_count", 0) != 0:
        raise _lib.M2TError(f"{what} in the middle of an accumulation cycle ({step.micro_count} of {step.accum_steps} "
                            "micro-batches since the last optimizer step)")


class TrainStep:
    # The state of the optional terms, off: what __init__ starts from and what a step object assembled without __init__ has.  A term
    # of LOSS_TERMS has its weight, its device [1] value and its per-shape scratch cache (None: the dict is made per object, on first
    # use or by the setter); the perceptual term keeps its value next to the PerceptualLoss object, whose workspace is its own.
    lambda_ssim = lambda_msssim = lambda_fft = lambda_vif = lambda_gmsd = lambda_wavelet = lambda_consistency = lambda_perceptual = 0.0
    ssim_loss = msssim_loss = fft_loss = vif_loss = gmsd_loss = wavelet_loss = consistency_loss = perceptual_loss_value = None
    _ssim_scratch = _msssim_scratch = _fft_scratch = _vif_scratch = _gmsd_scratch = _wavelet_scratch = _consistency_scratch = None
    wavelet, wavelet_levels, wavelet_band_weights, wavelet_eps = "haar", 2, None, 0.0
    _wavelet_call = None          # the C arguments of the wavelet term, made by the setter or on first use
    fft_norm = "backward"
    consistency_eps = 0.0
    perceptual_loss = None
    groups = None
    _need_stage = None
    track_health = 0              # record the step health every K-th step (M2Trans.track_health); 0 = off

    def __init__(self, model: M2Trans, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 lambda_l1: float = 1.0, process_group=None, world_size: Optional[int] = None,
                 grad_bucket_dtype: torch.dtype = torch.float32, semantic_loss=None, lambda_clip: float = 0.0,
                 overlap_comm: bool = True, force_comm_path: bool = False, overlap_semantic: bool = True,
                 accum_steps: int = 1, max_grad_norm: Optional[float] = None, weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, ema_decay: Optional[float] = None, skip_nonfinite: bool = False,
                 track_grad_norm: bool = False, pixel_loss: str = "l1", pixel_loss_param: Optional[float] = None,
                 lambda_ssim: float = 0.0, lambda_fft: float = 0.0, fft_norm: str = "backward",
                 lambda_msssim: float = 0.0, lambda_vif: float = 0.0, param_groups=None, perceptual_loss=None,
                 lambda_perceptual: float = 0.0, lambda_gmsd: float = 0.0, lambda_wavelet: float = 0.0, wavelet="haar",
                 wavelet_levels: int = 2, wavelet_band_weights=None, wavelet_eps: float = 0.0, lambda_consistency: float = 0.0,
                 consistency_eps: float = 0.0, track_health: int = 0):
        self.model = model
        # the step health record (M2Trans.track_health, level 2) on the steps with step_count % track_health == 0; 0 = off: the
        # plans are laid out and launched as before
        if int(track_health) != track_health or int(track_health) < 0:
            raise _lib.M2TError(f"track_health must be an integer >= 0 (record every K-th step; 0 = off), got {track_health!r}")
        self.track_health = int(track_health)
        if self.track_health:
            model.track_health(2)
            for key in [k for k, pl in (model._plans or {}).items() if not pl.inference and pl.query("opt:health") != 2]:
                del model._plans[key]               # (a training plan made before this object has no record: made again on first use)
        # parameter groups / frozen tensors (param_groups.py): resolved against the model's names here, on the host, fixed for the
        # life of this object.  None (the default): nothing is allocated and the step issues the calls it always issued
        self.groups = resolve_param_groups(model, param_groups)
        # the pixel term: lambda_l1 (the reference's config key) stays its weight and l1_loss the tensor that holds it, whatever the kind
        self.set_pixel_loss(pixel_loss, pixel_loss_param)
        # the optional terms, each lambda * (its measure): 0 = off (nothing allocated, the step issues the calls it always issued)
        self.set_lambda_ssim(lambda_ssim)
        self.set_lambda_msssim(lambda_msssim)
        self.set_lambda_fft(lambda_fft, fft_norm)
        self.set_lambda_vif(lambda_vif)
        self.set_lambda_gmsd(lambda_gmsd)
        self.set_lambda_wavelet(lambda_wavelet, wavelet, wavelet_levels, wavelet_band_weights, wavelet_eps)
        self.set_lambda_consistency(lambda_consistency, consistency_eps)
        self.perceptual_loss = perceptual_loss
        self.set_lambda_perceptual(lambda_perceptual)
        # gradient accumulation: one optimizer step consumes accum_steps equal micro-batches (forward_backward calls); the
        # gradients and the loss of calls 2..k of a cycle are added to the first call's by m2t_grad_accumulate
        if int(accum_steps) != accum_steps or int(accum_steps) < 1:
            raise _lib.M2TError(f"accum_steps must be an integer >= 1, got {accum_steps!r}")
        self.accum_steps = int(accum_steps)
        self.micro_count = 0                    # forward_backward calls since the last optimizer step (stays 0 with accum_steps = 1)
        # the SemanticLoss forward needs only sr (final after m2t_forward): it runs on its own stream under the backward pass
        self.overlap_semantic = bool(overlap_semantic)
        self.sem_stream = None
        self.lr = float(lr)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.lambda_l1 = float(lambda_l1)
        # the MedCLIP regulariser (train.py:78,203-205): a no-grad constant added to the logged loss, or -- with
        # SemanticLoss(differentiable=True) -- a term whose gradient reaches the weights (_forward_backward_semantic_grad)
        self.semantic_loss = semantic_loss
        self.lambda_clip = float(lambda_clip)
        self.clip_loss = None
        self.pg = process_group
        if world_size is None:
            world_size = torch.distributed.get_world_size(process_group) if (
                torch.distributed.is_available() and torch.distributed.is_initialized()) else 1
        self.world_size = int(world_size)
        self.step_count = 0
        self.scheduler_last_epoch = 0          # CosineAnnealingLR.last_epoch of the run (checkpoint.py keeps it across save / resume)
        flat = model.flat_params
        if not flat.is_cuda:
            raise _lib.M2TError("TrainStep needs the model on a HIP device (model.to('cuda'))")
        self.grads = model.attach_flat_grads()
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.l1_loss = torch.zeros(1, dtype=torch.float32, device=flat.device)
        self.loss = self.l1_loss
        # where micro-batches 2..k of a cycle put their gradients and their L1 loss (nothing is allocated for accum_steps = 1)
        # (with frozen tensors a partial backward pass never writes their ranges: zeros, not stale memory, for whoever looks at them)
        frozen_any = self.groups is not None and self.groups.any_frozen
        self.micro_grads = (torch.zeros_like(self.grads) if frozen_any else torch.empty_like(self.grads)) if self.accum_steps > 1 else None
        self.micro_loss = torch.zeros(1, dtype=torch.float32, device=flat.device) if self.accum_steps > 1 else None
        # force_comm_path: build the exchange machinery even for one rank (tests exercise the stream / event logic)
        self.bucket = GradBucket(self.grads, process_group, grad_bucket_dtype, force=force_comm_path,
                                 expect_world=self.world_size) if (self.world_size > 1 or force_comm_path) else None
        # overlapped exchange for either wire format (a bf16 wire stages each range through a slice of the wire buffer)
        self.overlap_comm = bool(overlap_comm) and self.bucket is not None
        self.comm_stream = _shared_stream(flat.device, "comm") if self.overlap_comm else None
        self._last_plan = None
        # bench.py / audits: with measure_exposed_comm the compute stream's wait for the gradient exchange is bracketed by two
        # timing events per step (exposed_comm_events: [(before, after)]) -- what the exchange costs the step after the overlap
        self.measure_exposed_comm = False
        self.exposed_comm_events = []
        self._init_optim_options(max_grad_norm, weight_decay, decoupled_weight_decay, ema_decay, skip_nonfinite, track_grad_norm)
        self._init_groups()

    def _init_groups(self):
        """The device copy of the segment table (uploaded ONCE, here), the frozen flags and the stage flags of the backward pass."""
        self._group_table = self._group_frozen = self._need_stage = None
        g = self.groups
        if g is None:
            return
        flat = self.model.flat_params
        if flat.numel() != g.n:
            raise _lib.M2TError(f"param_groups: resolved for {g.n} elements, the flat buffer holds {flat.numel()}")
        self._group_table = torch.frombuffer(bytearray(g.pack()), dtype=torch.uint8).to(flat.device)
        self._group_frozen = (C.c_ubyte * g.n_groups)(*[1 if f else 0 for f in g.frozen])
        if not all(g.stage_flags):
            # a stage with any trainable tensor still computes all its gradients; a stage without one does no parameter-gradient work
            self._need_stage = (C.c_ubyte * len(g.stage_flags))(*[1 if f else 0 for f in g.stage_flags])
        if g.any_frozen:
            self.grads.zero_()

    def _backward_call(self, lib, plan, lr_img, grads, ws, st):
        """m2t_backward, or -- when a whole stage is frozen -- m2t_backward_ex with the stage flags of the groups.  A deferred pixel
        loss survives a partial pass: it is taken in front of the first fork (or inside the fused tail backward, which runs for
        its data gradient whatever the tail's flag says) before any stage flag is looked at."""
        m = self.model
        if self._need_stage is None:
            _lib.check(lib.m2t_backward(plan.handle, _lib.ptr(m.flat_params), _lib.ptr(lr_img), _lib.ptr(grads),
                                        ws, st), "m2t_backward")
            return
        _lib.check(lib.m2t_backward_ex(plan.handle, _lib.ptr(m.flat_params), _lib.ptr(lr_img), _lib.ptr(grads), None,
                                       self._need_stage, ws, st), "m2t_backward_ex")

    def _init_optim_options(self, max_grad_norm, weight_decay, decoupled_weight_decay, ema_decay, skip_nonfinite, track_grad_norm):
        """Gradient-norm clipping, weight decay, EMA weights and the non-finite skip (m2t_grad_norm + m2t_adam_step_ex).  With
        every option off nothing is allocated and optimizer_step() stays the single m2t_adam_step call."""
        if max_grad_norm is not None and not (float(max_grad_norm) > 0.0 and math.isfinite(float(max_grad_norm))):
            raise _lib.M2TError(f"max_grad_norm must be None or a finite number > 0, got {max_grad_norm!r}")
        if not (float(weight_decay) >= 0.0 and math.isfinite(float(weight_decay))):
            raise _lib.M2TError(f"weight_decay must be a finite number >= 0, got {weight_decay!r}")
        if ema_decay is not None and not (0.0 <= float(ema_decay) < 1.0):
            raise _lib.M2TError(f"ema_decay must be None or in [0, 1), got {ema_decay!r}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.weight_decay = float(weight_decay)
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.track_grad_norm = bool(track_grad_norm)
        flat = self.model.flat_params
        # the optimizer record (include/m2t.h, m2t_grad_norm): 8 doubles on the device, written by the norm's second stage
        self._use_norm = self.max_grad_norm is not None or self.skip_nonfinite or self.track_grad_norm
        self.optim_record = self._norm_ws = None
        self.grad_norm = self.clip_coef = self.skipped_steps = None
        if self._use_norm:
            self.optim_record = torch.zeros(8, dtype=torch.float64, device=flat.device)
            self._norm_ws = torch.empty(int(_lib.load().m2t_grad_norm_workspace_bytes()) // 8, dtype=torch.float64, device=flat.device)
            # views of the record: reading one is the caller's synchronisation, at the caller's cadence
            self.grad_norm, self.clip_coef, self.skipped_steps = self.optim_record[0], self.optim_record[2], self.optim_record[4]
        self.ema_params = flat.detach().clone() if self.ema_decay is not None else None
        self._optim_ex = self._use_norm or self.weight_decay != 0.0 or self.ema_params is not None

    def set_pixel_loss(self, name, param=None):
        """Choose the pixel loss: 'l1', 'mse' (alias 'l2'), 'charbonnier' (param = eps, default 1e-6), 'smooth_l1' (alias 'sl1';
        param = beta, default 1.0).  Takes effect with the next forward_backward (checkpoint.import_checkpoint calls this)."""
        _refuse_mid_cycle(self, "set_pixel_loss")
        self._pixel_kind, self.pixel_loss, self.pixel_loss_param = resolve_pixel_loss(name, param)

    # -- the optional terms of LOSS_TERMS: one setter, one scratch cache and one call for all of them -----------------------
    def _set_lambda(self, term: LossTerm, value):
        """Weight of one term (0 = off): the [1] value exists while the term is on; turning it off drops value and scratch."""
        n = term.name
        _refuse_mid_cycle(self, f"set_lambda_{n}")
        lam = resolve_lambda(n, value)
        setattr(self, f"lambda_{n}", lam)
        if lam > 0.0:
            if getattr(self, f"{n}_loss") is None:
                setattr(self, f"{n}_loss", torch.zeros(1, dtype=torch.float32, device=self.model.flat_params.device))
        else:
            setattr(self, f"{n}_loss", None)
            setattr(self, f"_{n}_scratch", {})

    def set_lambda_ssim(self, value):
        """Weight of the structural term (0 = off).  Takes effect with the next forward_backward (checkpoint.import_checkpoint
        calls this); refused in the middle of an accumulation cycle."""
        self._set_lambda(_TERM["ssim"], value)

    def set_lambda_msssim(self, value):
        """Weight of the multi-scale structural term (0 = off).  Takes effect with the next forward_backward
        (checkpoint.import_checkpoint calls this); refused in the middle of an accumulation cycle."""
        self._set_lambda(_TERM["msssim"], value)

    def set_lambda_fft(self, value, norm=None):
        """Weight of the frequency-domain term (0 = off) and, when given, its normalisation ('backward' / 'ortho').  Takes effect
        with the next forward_backward (checkpoint.import_checkpoint calls this); refused in the middle of an accumulation cycle."""
        _refuse_mid_cycle(self, "set_lambda_fft")
        lam = resolve_lambda("fft", value)      # (a refused weight leaves the normalisation as it was)
        if norm is not None:
            self.fft_norm = resolve_fft_norm(norm)
        self._set_lambda(_TERM["fft"], lam)

    def set_lambda_vif(self, value):
        """Weight of the information-fidelity term (0 = off).  Takes effect with the next forward_backward
        (checkpoint.import_checkpoint calls this); refused in the middle of an accumulation cycle."""
        self._set_lambda(_TERM["vif"], value)

    def set_lambda_gmsd(self, value):
        """Weight of the GMSD term (0 = off).  Takes effect with the next forward_backward (checkpoint.import_checkpoint calls
        this); refused in the middle of an accumulation cycle."""
        self._set_lambda(_TERM["gmsd"], value)

    def set_lambda_wavelet(self, value, wavelet=None, levels=None, band_weights=None, eps=None):
        """Weight of the wavelet-domain term (0 = off) and, where given, its filter pair ('haar', 'db2' or (lo, hi)), level count
        (1 .. 3), band weights (3 levels + 1 numbers: three detail bands per level, then LL) and eps (0 = L1, > 0 = Charbonnier);
        None keeps what the step has.  Takes effect with the next forward_backward (checkpoint.import_checkpoint calls this);
        refused in the middle of an accumulation cycle."""
        _refuse_mid_cycle(self, "set_lambda_wavelet")
        lam = resolve_lambda("wavelet", value)      # (a refused weight or argument leaves the step as it was)
        w = resolve_wavelet(self.wavelet if wavelet is None else wavelet, self.wavelet_levels if levels is None else levels,
                            self.wavelet_band_weights if band_weights is None else band_weights,
                            self.wavelet_eps if eps is None else eps)
        self.wavelet, self.wavelet_levels, self.wavelet_eps = w.wavelet, w.levels, w.eps
        self.wavelet_band_weights = None if w.band_weights is None else list(w.band_weights)
        self._wavelet_call = wavelet_call_args(w) if lam > 0.0 else None
        self._wavelet_scratch = {}                  # (sized by the level count)
        self._set_lambda(_TERM["wavelet"], lam)

    def _wavelet_args(self) -> tuple:
        if self._wavelet_call is None:
            self._wavelet_call = wavelet_call_args(resolve_wavelet(self.wavelet, self.wavelet_levels, self.wavelet_band_weights,
                                                                   self.wavelet_eps))
        return self._wavelet_call

    def _wavelet_shape_args(self) -> tuple:
        a = self._wavelet_args()
        return a[3], a[2]                           # levels, taps

    def set_lambda_consistency(self, value, eps=None):
        """Weight of the LR-consistency term (0 = off) and, when given, its eps (0 = L1, > 0 = Charbonnier): ``lambda_consistency *
        mean rho((D(clamp(sr)) - lr) / rgb_range)`` over the LR elements, D the bicubic down-sampler of the model's scale
        (m2t_consistency_loss of include/m2t_consistency.h); the target is the step's own ``lr_img``.  Takes effect with the next
        forward_backward (checkpoint.import_checkpoint calls this); refused in the middle of an accumulation cycle."""
        _refuse_mid_cycle(self, "set_lambda_consistency")
        lam = resolve_lambda("consistency", value)      # (a refused weight leaves eps as it was)
        if eps is not None:
            self.consistency_eps = resolve_consistency_eps(eps)
        self._set_lambda(_TERM["consistency"], lam)

    def _scratch_for(self, term: LossTerm, lib, img):
        """The scratch of one term for this (micro-)batch shape, allocated once; img is the term's target (hr_img, or lr_img for the
        consistency term).  A size the term does not take is refused here, on the host, before anything is launched."""
        n = term.name
        B, _, Hs, Ws = img.shape
        cache = getattr(self, f"_{n}_scratch")
        if cache is None:
            cache = {}
            setattr(self, f"_{n}_scratch", cache)
        more = term.shape_args(self)
        key = (B, Hs, Ws) + more
        if key not in cache:
            if not term.size_ok(Hs, Ws, *more):
                raise _lib.M2TError(f"lambda_{n} > 0: " + term.too_small.format(B=B, Hs=Hs, Ws=Ws))
            tail = term.scratch_tail(self)
            nbytes = int(getattr(lib, term.scratch_entry or f"m2t_{n}_loss_scratch_bytes")(B, 3, Hs, Ws, *more, *tail))
            if nbytes == 0:
                raise _lib.M2TError(f"lambda_{n} > 0: " + term.no_scratch.format(*tail, B=B, Hs=Hs, Ws=Ws))
            cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        return cache[key]

    @staticmethod
    def _store_or_add(first: bool) -> int:
        """The accumulate flag of every m2t_*_loss call: a term's value is stored by the first micro-batch of a cycle and added to
        by the others."""
        return 0 if first else 1

    def _term_call(self, term: LossTerm, lib, img, plan, first: bool, ws, st):
        """m2t_<n>_loss of one (micro-)batch against the term's target img, behind the immediate pixel loss and the terms in front of
        it: adds into the materialised seed.  The divisor is the GLOBAL count of what the term's mean runs over."""
        n = term.name
        B, _, Hs, Ws = img.shape
        divisor = global_divisor(term.count(B, Hs, Ws), self.world_size, self.accum_steps)
        entry = f"m2t_{n}_loss"
        _lib.check(getattr(lib, entry)(plan.handle, _lib.ptr(img), getattr(self, f"lambda_{n}"), divisor, float(self.model.rgb_range),
                                       *term.extra(self), _lib.ptr(getattr(self, f"{n}_loss")), self._store_or_add(first),
                                       _lib.ptr(self._scratch_for(term, lib, img)), ws, st), entry)

    # -- the perceptual term: the same slot in the order and in the total, its own preconditions, workspace and call ---------------
    def set_lambda_perceptual(self, value):
        """Weight of the VGG19 feature term (0 = off); needs ``perceptual_loss=`` (a losses.PerceptualLoss with weights loaded, resize
        off, data_range = the model's rgb_range).  Takes effect with the next forward_backward; refused in the middle of an
        accumulation cycle."""
        _refuse_mid_cycle(self, "set_lambda_perceptual")
        self.lambda_perceptual = resolve_lambda("perceptual", value)
        if self.lambda_perceptual > 0.0:
            p = self.perceptual_loss
            if p is None:
                raise _lib.M2TError("lambda_perceptual > 0 needs perceptual_loss= (a losses.PerceptualLoss with VGG19 weights loaded)")
            if not p.loaded:
                raise _lib.M2TError("lambda_perceptual > 0: the PerceptualLoss has no VGG19 weights loaded (none ship): call load_vgg_state_dict first")
            if p.resize:
                raise _lib.M2TError("lambda_perceptual > 0: resize=True is not built into the training step (use resize=False)")
            if float(p.data_range) != float(self.model.rgb_range):
                raise _lib.M2TError(f"lambda_perceptual > 0: the PerceptualLoss's data_range {p.data_range} is not the model's rgb_range "
                                    f"{self.model.rgb_range}")
            if self.perceptual_loss_value is None:
                self.perceptual_loss_value = torch.zeros(1, dtype=torch.float32, device=self.model.flat_params.device)
        else:
            self.perceptual_loss_value = None

    def _perceptual_workspace_for(self, hr_img):
        """The tower's workspace for this (micro-)batch shape (cached by the PerceptualLoss object); an SR size below 16 is refused
        here, on the host, before anything is launched."""
        B, _, Hs, Ws = hr_img.shape
        if not perceptual_size_supported(Hs, Ws):
            raise _lib.M2TError(f"lambda_perceptual > 0: the SR image {Hs}x{Ws} is too small (height and width must be at least 16: four "
                                "pools before relu5_1)")
        return self.perceptual_loss.workspace(B, Hs, Ws, True)

    def _perceptual_loss_call(self, lib, hr_img, plan, first: bool, ws, st):
        """m2t_vgg_loss of one (micro-)batch, behind the immediate pixel loss and the other terms: adds into the materialised seed."""
        p = self.perceptual_loss
        divisor = global_divisor(hr_img.shape[0], self.world_size, self.accum_steps)     # global number of images
        _lib.check(lib.m2t_vgg_loss(plan.handle, p.handle, _lib.ptr(hr_img), self.lambda_perceptual, divisor, float(self.model.rgb_range),
                                    p.kind, p.param, p.tap_weights(), _lib.ptr(self.perceptual_loss_value), self._store_or_add(first),
                                    _lib.ptr(self._perceptual_workspace_for(hr_img)), ws, st), "m2t_vgg_loss")

    # -- what forward_backward iterates ------------------------------------------------------------------------------------
    def _terms_on(self, lib, lr_img, hr_img) -> list:
        """The optional terms that are on, in call order -- the rows of LOSS_TERMS, then the perceptual term -- each as (value,
        prepare, call) bound to its target image of this (micro-)batch: the term's device [1] tensor; prepare(), which refuses a size
        the term does not take and makes sure of its scratch before anything is launched; call(plan, first, ws, st), its m2t_*_loss
        call."""
        images = {"lr_img": lr_img, "hr_img": hr_img}
        on = [(getattr(self, f"{t.name}_loss"), functools.partial(self._scratch_for, t, lib, images[t.target]),
               functools.partial(self._term_call, t, lib, images[t.target]))
              for t in LOSS_TERMS if getattr(self, f"lambda_{t.name}") > 0.0]
        if self.lambda_perceptual > 0.0:
            on.append((self.perceptual_loss_value, functools.partial(self._perceptual_workspace_for, hr_img),
                       functools.partial(self._perceptual_loss_call, lib, hr_img)))
        return on

    def _total_loss(self, on: list, with_clip: bool):
        loss = self.l1_loss
        for value, _, _ in on:
            loss = loss + value
        return loss + self.clip_loss if with_clip else loss

    def _pixel_loss_call(self, lib, deferred: bool, plan, hr_img, divisor, l1_loss, ws, st):
        """The loss + seed request of one (micro-)batch.  'l1' calls the entry points it always called."""
        m = self.model
        if self._pixel_kind == 0:
            fn, what = (lib.m2t_l1_loss_deferred, "m2t_l1_loss_deferred") if deferred else (lib.m2t_l1_loss, "m2t_l1_loss")
            _lib.check(fn(plan.handle, _lib.ptr(hr_img), self.lambda_l1, divisor, float(m.rgb_range), _lib.ptr(l1_loss), ws, st), what)
            return
        fn, what = (lib.m2t_pixel_loss_deferred, "m2t_pixel_loss_deferred") if deferred else (lib.m2t_pixel_loss, "m2t_pixel_loss")
        _lib.check(fn(plan.handle, self._pixel_kind, self.pixel_loss_param or 0.0, _lib.ptr(hr_img), self.lambda_l1, divisor,
                      float(m.rgb_range), _lib.ptr(l1_loss), ws, st), what)

    def applied_step_count(self) -> int:
        """step_count minus the optimizer steps skip_nonfinite left out (Adam's effective step number).  Synchronises."""
        return self.step_count - (int(self.skipped_steps.item()) if self.skipped_steps is not None else 0)

    def _need_ema(self, what: str):
        if self.ema_params is None:
            raise _lib.M2TError(f"{what}: this TrainStep keeps no EMA weights (ema_decay=None)")

    def ema_state_dict(self) -> dict:
        """The EMA weights under the model's own state_dict names (the frozen MeanShift entries are the model's), as copies:
        ``model.load_state_dict(ts.ema_state_dict(), strict=True)`` works."""
        self._need_ema("ema_state_dict")
        from .checkpoint import ema_state_dict
        return ema_state_dict(self.model, self.ema_params)

    def swap_ema(self):
        """Exchange the contents of model.flat_params and ema_params in place (a validation sweep between epochs runs the model on
        the EMA weights, a second call puts every bit back).  Plain torch copies: this is off the timed path."""
        self._need_ema("swap_ema")
        _refuse_mid_cycle(self, "swap_ema")
        flat = self.model.flat_params
        with torch.no_grad():
            tmp = flat.detach().clone()
            flat.copy_(self.ema_params)
            self.ema_params.copy_(tmp)

    def set_lr(self, lr: float):
        self.lr = float(lr)

    # -- pieces (also used by tests) -------------------------------------------------------
    def forward_backward(self, lr_img: torch.Tensor, hr_img: torch.Tensor, captions=None) -> torch.Tensor:
        """forward + the pixel loss (L1 by default) (+ the constant SemanticLoss term) + backward into model.flat_grads; returns the
        device loss tensor (this rank's share of the global mean).  With accum_steps = k > 1 this is ONE micro-batch: the first
        call of a cycle fills model.flat_grads and the loss, calls 2..k add to them (in call order, fp32), and a call beyond the
        k-th before optimizer_step() raises."""
        first = self.micro_count == 0
        if self.accum_steps > 1 and self.micro_count >= self.accum_steps:
            raise _lib.M2TError(f"forward_backward: {self.micro_count} micro-batches since the last optimizer step, accum_steps is "
                                f"{self.accum_steps}: call all_reduce_grads() / optimizer_step() first")
        m = self.model
        lib = _lib.load()
        plan = m._plan_for(lr_img)
        lr_img = lr_img.contiguous().float()
        hr_img = hr_img.contiguous().float()
        B = lr_img.shape[0]
        if tuple(hr_img.shape) != (B, 3, lr_img.shape[2] * m.scale, lr_img.shape[3] * m.scale):
            raise _lib.M2TError("hr shape must be [B,3,H*scale,W*scale]")
        on = self._terms_on(lib, lr_img, hr_img)
        for _, prepare, _ in on:
            prepare()                               # (refuses an SR size the term does not take before any launch)
        divisor = global_divisor(hr_img.numel(), self.world_size, self.accum_steps)      # global mean (equal shards, equal micro-batches)
        use_clip = self.semantic_loss is not None and self.lambda_clip > 0 and captions is not None
        # (micro-batches 2..k of a cycle: a second gradient buffer and a second loss slot, added to the first ones below)
        grads = self.grads if first else self.micro_grads
        l1_loss = self.l1_loss if first else self.micro_loss
        if use_clip and getattr(self.semantic_loss, "differentiable", False):
            return self._forward_backward_semantic_grad(m, lib, plan, lr_img, hr_img, captions, divisor, grads, l1_loss, on)
        sr = torch.empty_like(hr_img) if use_clip else None
        plan.gen += 1
        plan.trained = True              # (the plan LRU of the model keeps training plans while forward-only ones remain)
        self._last_plan = plan
        self._health_switch(lib, plan)
        with torch.cuda.device(lr_img.device):
            st = _lib.stream_ptr()
            ws = _lib.ptr(plan.workspace)
            _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(m.flat_params), _lib.ptr(lr_img), _lib.ptr(sr),
                                       float(m.rgb_range), 1, ws, st), "m2t_forward")
            # (deferred: the loss and the backward seed are produced inside m2t_backward, which follows at once -- on the bf16 x4
            #  path by the fused tail backward itself; hr_img stays alive until then)
            # (any optional term on: the materialised seed -- the immediate pixel loss, then each term added into it, in the order
            #  of _terms_on)
            self._pixel_loss_call(lib, not on, plan, hr_img, divisor, l1_loss, ws, st)
            for _, _, call in on:
                call(plan, first, ws, st)
            fwd_done = torch.cuda.current_stream(lr_img.device).record_event() if (use_clip and self.overlap_semantic) else None
            self._backward_call(lib, plan, lr_img, grads, ws, st)
            self._accumulate_micro(lib, first, st)
        if use_clip:
            # clip_loss += loss_clip(sr[i], hr[i], caption_i) * lambda_clip  (train.py:203-205); no gradient
            if self.overlap_semantic:
                # the backward pass is already enqueued on the caller's stream; the encoder (which synchronises its own
                # stream once for the crop table) follows the forward pass on a second stream and is joined afterwards
                main = torch.cuda.current_stream(lr_img.device)
                if self.sem_stream is None:
                    # (normal priority: PyTorch-ROCm exposes no priority below the default one)
                    self.sem_stream = _shared_stream(lr_img.device, "semantic")
                self.sem_stream.wait_event(fwd_done)
                with torch.cuda.stream(self.sem_stream):
                    self._add_clip(self.semantic_loss.batch(sr, hr_img, captions) * self.lambda_clip, first)
                main.wait_stream(self.sem_stream)
            else:
                self._add_clip(self.semantic_loss.batch(sr, hr_img, captions) * self.lambda_clip, first)
        self.loss = self._total_loss(on, use_clip)
        return self.loss

    def _health_switch(self, lib, plan):
        """track_health = K: the record's launches run on the steps with step_count % K == 0 (with accum_steps, on the last
        micro-batch of such a step); on every other pass option "health_on" is 0 and the pass adds no launch.  Host state only."""
        if not self.track_health:
            return
        on = self.step_count % self.track_health == 0 and self.micro_count == self.accum_steps - 1
        if getattr(plan, "health_on", True) != on:
            _lib.check(lib.m2t_set_option(plan.handle, b"health_on", int(on)), "m2t_set_option(health_on)")
            plan.health_on = on

    def health(self):
        """The ``HealthReport`` of the last recorded step (m2trans_amd/health.py): ``.first_nonfinite`` names the stage where a NaN
        or Inf first appeared -- what to read after ``skipped_steps`` grows.  Synchronises."""
        from .health import HealthReport
        if not self.track_health:
            raise _lib.M2TError("TrainStep.health: made with track_health = 0 (off)")
        if self._last_plan is None:
            raise _lib.M2TError("TrainStep.health: no step has run yet")
        return HealthReport.from_plan(self._last_plan)

    def _accumulate_micro(self, lib, first: bool, st):
        """Close one micro-batch: count it and, from the second one of a cycle on, grads += micro_grads, l1_loss += micro_loss."""
        if self.accum_steps == 1:
            return
        self.micro_count += 1
        if first:
            return
        # no event needed: m2t_backward ends with its side stream joined into the caller's stream (every gradient and the deferred
        # loss are complete in the order of that stream), and the next micro-batch's side-stream launches are forked from this
        # stream behind this kernel -- the ordering Adam and the next step's backward rely on today
        _lib.check(lib.m2t_grad_accumulate(_lib.ptr(self.grads), _lib.ptr(self.micro_grads), self.grads.numel(),
                                           _lib.ptr(self.l1_loss), _lib.ptr(self.micro_loss), st), "m2t_grad_accumulate")

    def _add_clip(self, clip: torch.Tensor, first: bool):
        """The SemanticLoss term of one micro-batch (a per-sample SUM: no divisor) into the cycle's clip_loss."""
        self.clip_loss = clip if first else self.clip_loss + clip

    def _forward_backward_semantic_grad(self, m, lib, plan, lr_img, hr_img, captions, divisor, grads, l1_loss, on):
        """The route of a differentiable SemanticLoss: forward -> semantic encode (the SR crops stash what the encoder's backward
        needs, the HR crops do not) -> its vector-Jacobian product -> m2t_l1_loss (a MATERIALISED seed: the fused-L1 seed of the
        default route, m2t_l1_loss_deferred, does not apply here) -> m2t_add_output_grad(lambda_clip) -> m2t_backward.  HIP kernels
        only, one stream.  The semantic term is a per-sample SUM on every rank, so a SUM all-reduce of the gradients equals the
        gradient of the global-batch sum without rescaling (as the reference's DataParallel gather)."""
        sl = self.semantic_loss
        first = grads is self.grads
        sr = torch.empty_like(hr_img)
        plan.gen += 1
        plan.trained = True
        self._last_plan = plan
        self._health_switch(lib, plan)
        with torch.cuda.device(lr_img.device):
            st = _lib.stream_ptr()
            ws = _lib.ptr(plan.workspace)
            _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(m.flat_params), _lib.ptr(lr_img), _lib.ptr(sr),
                                       float(m.rgb_range), 1, ws, st), "m2t_forward")
            tot, g, origins = sl._value_and_grad(sr, hr_img, captions)
            self._pixel_loss_call(lib, False, plan, hr_img, divisor, l1_loss, ws, st)
            for _, _, call in on:
                call(plan, first, ws, st)
            g = g.contiguous()
            arr = None
            if origins is not None:
                arr = (C.c_int * (2 * len(origins)))(*[int(v) for o in origins for v in o])
            _lib.check(lib.m2t_add_output_grad(plan.handle, _lib.ptr(g), g.shape[2], g.shape[3], arr, self.lambda_clip,
                                               float(m.rgb_range), ws, st), "m2t_add_output_grad")
            self._backward_call(lib, plan, lr_img, grads, ws, st)
            self._accumulate_micro(lib, first, st)
        self._add_clip(tot * self.lambda_clip, first)
        self.loss = self._total_loss(on, True)
        return self.loss

    def all_reduce_grads(self):
        """SUM the gradients over the ranks.  Overlapped mode: m2t_backward (already enqueued) completes the flat
        buffer in contiguous buckets (tail, block pairs from last to first, head); each bucket's all-reduce is
        enqueued on the communication stream behind that bucket's event, so it runs under the remaining backward
        kernels; the compute stream then waits for the communication stream (before Adam).  With accum_steps = k > 1 the
        exchange runs once per optimizer step, on the accumulated buffer, behind the last accumulate."""
        self._check_cycle_complete("all_reduce_grads")
        if self.bucket is None:
            return
        ev0 = None
        if self.measure_exposed_comm:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record(torch.cuda.current_stream(self.grads.device))
        self._all_reduce_grads()
        if ev0 is not None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record(torch.cuda.current_stream(self.grads.device))
            self.exposed_comm_events.append((ev0, ev1))

    def _all_reduce_grads(self):
        if not self.overlap_comm or self._last_plan is None:
            self.bucket.all_reduce()
            return
        lib = _lib.load()
        plan = self._last_plan
        main = torch.cuda.current_stream(self.grads.device)
        buckets = plan.grad_buckets()
        # two collectives: everything that is final once the third-last block pair has been reduced (the tail and
        # 3/4 of the body: its exchange runs under the last quarter of the backward pass), then the rest.  More,
        # smaller collectives cost more in launch latency than they hide (measured with one rank: +25 us each).
        cut = max(0, len(buckets) - 3)
        groups = [(cut, buckets[cut][0], buckets[0][1]), (len(buckets) - 1, 0, buckets[cut][0])] if cut > 0 else \
                 [(len(buckets) - 1, 0, buckets[0][1])]
        if self.accum_steps > 1:
            # the bucket events of the last micro-batch's backward describe the micro buffer, not the sum: the same two ranges,
            # behind the last m2t_grad_accumulate
            self.comm_stream.wait_stream(main)
        with torch.cuda.device(self.grads.device), torch.cuda.stream(self.comm_stream):
            for last, lo, hi in groups:
                if self.accum_steps == 1:
                    _lib.check(lib.m2t_stream_wait_bucket(plan.handle, last, self.comm_stream.cuda_stream), "m2t_stream_wait_bucket")
                self.bucket.all_reduce_range(lo, hi)
        main.wait_stream(self.comm_stream)

    def _check_cycle_complete(self, what: str):
        """accum_steps = k > 1: a partial sum scaled by the full divisor would train silently on a wrong gradient."""
        if self.accum_steps > 1 and self.micro_count != self.accum_steps:
            raise _lib.M2TError(f"{what}: {self.micro_count} of {self.accum_steps} micro-batches since the last optimizer step "
                                "(accum_steps): the gradient buffer does not hold the whole cycle")

    def optimizer_step(self):
        self._check_cycle_complete("optimizer_step")
        self.micro_count = 0                    # closes the cycle; step_count counts optimizer steps, never micro-batches
        self.step_count += 1
        lib = _lib.load()
        with torch.cuda.device(self.grads.device):
            if self.groups is not None:
                self._optimizer_step_groups(lib, _lib.stream_ptr())
                return
            if self._optim_ex:
                self._optimizer_step_ex(lib, _lib.stream_ptr())
                return
            _lib.check(lib.m2t_adam_step(_lib.ptr(self.model.flat_params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg),
                                         _lib.ptr(self.exp_avg_sq), self.grads.numel(), self.lr, self.betas[0],
                                         self.betas[1], self.eps, self.step_count, 1.0, _lib.stream_ptr()),
                       "m2t_adam_step")

    def _optimizer_step_ex(self, lib, st):
        """The step with options: the norm of the accumulated, all-reduced gradient (this runs behind the last accumulate and
        behind the wait for the communication stream, so every rank computes the same number and takes the same skip decision
        without a collective) into the record, then ONE pass that clips, decays, steps and updates the EMA -- or does nothing."""
        n = self.grads.numel()
        if self._use_norm:
            _lib.check(lib.m2t_grad_norm(_lib.ptr(self.grads), n, 1.0, self.max_grad_norm or 0.0, int(self.skip_nonfinite),
                                         self.step_count, self.betas[0], self.betas[1], _lib.ptr(self.optim_record),
                                         _lib.ptr(self._norm_ws), st), "m2t_grad_norm")
        _lib.check(lib.m2t_adam_step_ex(_lib.ptr(self.model.flat_params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg),
                                        _lib.ptr(self.exp_avg_sq), n, self.lr, self.betas[0], self.betas[1], self.eps,
                                        self.step_count, 1.0, _lib.ptr(self.ema_params), self.weight_decay,
                                        int(self.decoupled_weight_decay), self.ema_decay or 0.0, _lib.ptr(self.optim_record), st),
                   "m2t_adam_step_ex")

    def _optimizer_step_groups(self, lib, st):
        """The step with parameter groups: the norm over the trainable elements (if clip / skip / track is on) into the record,
        then ONE grouped pass.  Each group's lr / weight decay is evaluated here in Python floats and travels by value; the table
        is the device copy made at construction.  Nothing reads a frozen range of the gradient buffer."""
        g = self.groups
        n, ng = self.grads.numel(), g.n_groups
        table = _lib.ptr(self._group_table)
        if self._use_norm:
            _lib.check(lib.m2t_grad_norm_groups(_lib.ptr(self.grads), n, 1.0, self.max_grad_norm or 0.0, int(self.skip_nonfinite),
                                                self.step_count, self.betas[0], self.betas[1], _lib.ptr(self.optim_record),
                                                _lib.ptr(self._norm_ws), self._group_frozen, ng, table, g.n_seg, st),
                       "m2t_grad_norm_groups")
        lrs = (C.c_float * ng)(*g.group_lr(self.lr))
        wds = (C.c_float * ng)(*g.group_weight_decay(self.weight_decay))
        _lib.check(lib.m2t_adam_step_groups(_lib.ptr(self.model.flat_params), _lib.ptr(self.grads), _lib.ptr(self.exp_avg),
                                            _lib.ptr(self.exp_avg_sq), n, lrs, self.betas[0], self.betas[1], self.eps,
                                            self.step_count, 1.0, _lib.ptr(self.ema_params), wds, int(self.decoupled_weight_decay),
                                            self.ema_decay or 0.0, _lib.ptr(self.optim_record), self._group_frozen, ng, table,
                                            g.n_seg, st), "m2t_adam_step_groups")

    # -- the step ----------------------------------------------------------------------------
    def step(self, lr_img: torch.Tensor, hr_img: torch.Tensor, captions=None) -> torch.Tensor:
        """One optimizer step on one batch.  With accum_steps = k > 1 the batch holds k * b samples and is cut, in sample
        order, into k micro-batches of b (views of the batch), each run through the plan of the micro-batch shape."""
        if self.accum_steps > 1:
            return self._step_accumulated(lr_img, hr_img, captions)
        loss = self.forward_backward(lr_img, hr_img, captions)
        self.all_reduce_grads()
        self.optimizer_step()
        return loss

    def _step_accumulated(self, lr_img, hr_img, captions):
        k, B = self.accum_steps, int(lr_img.shape[0])
        if B == 0 or B % k:
            raise _lib.M2TError(f"step: a batch of {B} samples cannot be cut into accum_steps = {k} equal micro-batches")
        if int(hr_img.shape[0]) != B:
            raise _lib.M2TError(f"step: {B} LR samples but {int(hr_img.shape[0])} HR samples")
        if self.micro_count != 0:
            raise _lib.M2TError(f"step: {self.micro_count} of {k} micro-batches of a cycle are already in the gradient buffer")
        if captions is not None:
            captions = list(captions)
            if len(captions) != B:
                raise _lib.M2TError(f"step: {B} samples but {len(captions)} captions")
        b = B // k
        for i in range(k):
            loss = self.forward_backward(lr_img[i * b:(i + 1) * b], hr_img[i * b:(i + 1) * b],
                                         captions[i * b:(i + 1) * b] if captions is not None else None)
        self.all_reduce_grads()
        self.optimizer_step()
        return loss

