"""Y-channel PSNR exactly as the reference's eval loop computes it (host side, fp64).

Restates utils.rgb_to_ycbcr (utils.py:121-146; note the `/255` applied to inputs that are already
in [0,1]), the scale-pixel border crop and x255 of test.py:101-111 / train.py:299-309, and
utils.calc_psnr (utils.py:179-184)."""
from __future__ import annotations

import math

import torch


def rgb_to_y(img: torch.Tensor) -> torch.Tensor:
    img = img / 255.0
    return (65.481 * img[..., 0, :, :] + 128.553 * img[..., 1, :, :] + 24.966 * img[..., 2, :, :] + 16.0).unsqueeze(-3)


def calc_psnr(sr: torch.Tensor, hr: torch.Tensor) -> float:
    diff = (sr.double() - hr.double()) / 255.0
    return float(-10.0 * math.log10(float(diff.pow(2).mean())))


def psnr_y(sr: torch.Tensor, hr: torch.Tensor, scale: int, rgb_range: float = 1.0) -> float:
    s, h = rgb_to_y(sr), rgb_to_y(hr)
    s = s[..., scale:-scale, scale:-scale]
    h = h[..., scale:-scale, scale:-scale]
    if rgb_range == 1:
        s, h = s * 255.0, h * 255.0
    return calc_psnr(s, h)


_WINDOW = None


def _ssim_window() -> torch.Tensor:
    """11-tap Gaussian, sigma 1.5, evaluated and normalised in fp32 with torch ops exactly as `pytorch_msssim`
    builds its window (host tensor, read by m2t_eval_metrics during the call)."""
    global _WINDOW
    if _WINDOW is None:
        c = torch.arange(11, dtype=torch.float32) - 11 // 2
        g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
        _WINDOW = (g / g.sum()).contiguous()
    return _WINDOW


def y_metrics_device(sr: torch.Tensor, hr: torch.Tensor, scale: int, rgb_range: float = 1.0) -> torch.Tensor:
    """PSNR input and SSIM of the eval loop (test.py:101-113, utils.py:179-184,232-234) on the device:
    [B,3,H,W] float32 pairs -> float64 [B,2] = (mean squared Y error, mean SSIM) per image.  HIP kernels
    behind `m2t_eval_metrics` (k_metrics.hip); no host fallback for device tensors."""
    from . import _lib
    if sr.shape != hr.shape or sr.dim() != 4 or sr.shape[1] != 3:
        raise _lib.M2TError(f"expected two [B,3,H,W] tensors of equal shape, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    if not (sr.is_cuda and hr.is_cuda):
        raise _lib.M2TError("y_metrics_device needs HIP device tensors (use psnr_y for host tensors)")
    lib = _lib.load()
    sr, hr = sr.contiguous().float(), hr.contiguous().float()
    B, _, H, W = sr.shape
    nbytes = lib.m2t_eval_metrics_scratch_bytes(B, H, W, scale)
    if nbytes == 0:
        raise _lib.M2TError(f"image {H}x{W} is too small for a border crop of {scale}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=sr.device)
    out = torch.empty(B, 2, dtype=torch.float64, device=sr.device)
    with torch.cuda.device(sr.device):
        _lib.check(lib.m2t_eval_metrics(_lib.ptr(sr), _lib.ptr(hr), B, H, W, scale, float(rgb_range), _ssim_window().data_ptr(),
                                        _lib.ptr(scratch), _lib.ptr(out), _lib.stream_ptr()), "m2t_eval_metrics")
    return out


def gmsd_device(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """``piq.gmsd(x, y, data_range=data_range, reduction='none')`` (test.py:98) on the device: [B,3,H,W] float32 pairs ->
    float64 [B].  HIP kernels behind `m2t_eval_gmsd` (k_metrics.hip); parity unpinned (`piq` is not vendored)."""
    from . import _lib
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
        raise _lib.M2TError(f"expected two [B,3,H,W] tensors of equal shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if not (x.is_cuda and y.is_cuda):
        raise _lib.M2TError("gmsd_device needs HIP device tensors")
    lib = _lib.load()
    x, y = x.contiguous().float(), y.contiguous().float()
    B, _, H, W = x.shape
    scratch = torch.empty(lib.m2t_eval_gmsd_scratch_bytes(B), dtype=torch.uint8, device=x.device)
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.m2t_eval_gmsd(_lib.ptr(x), _lib.ptr(y), B, H, W, float(data_range), _lib.ptr(scratch), _lib.ptr(out),
                                     _lib.stream_ptr()), "m2t_eval_gmsd")
    return out


def fsim_device(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """``piq.fsim(x, y, data_range=data_range, reduction='none')`` (test.py:95; FSIMc, piq 0.8.0 defaults) on the device: [B,3,H,W]
    float32 pairs -> float64 [B].  HIP kernels behind `m2t_eval_fsim` (k_fsim.hip); parity unpinned (`piq` is not vendored)."""
    from . import _lib
    if x.shape != y.shape or x.dim() != 4 or x.shape[1] != 3:
        raise _lib.M2TError(f"expected two [B,3,H,W] tensors of equal shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if not (x.is_cuda and y.is_cuda):
        raise _lib.M2TError("fsim_device needs HIP device tensors")
    lib = _lib.load()
    x, y = x.contiguous().float(), y.contiguous().float()
    B, _, H, W = x.shape
    nbytes = lib.m2t_eval_fsim_scratch_bytes(H, W)
    if nbytes == 0:
        raise _lib.M2TError(f"image {H}x{W} is too small for FSIM")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.m2t_eval_fsim(_lib.ptr(x), _lib.ptr(y), B, H, W, float(data_range), _lib.ptr(scratch), _lib.ptr(out),
                                     _lib.stream_ptr()), "m2t_eval_fsim")
    return out


def ms_ssim_device(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """``pytorch_msssim.ms_ssim(x, y, data_range=data_range, size_average=False)`` / ``piq.multi_scale_ssim(..., reduction='none')``
    on the device: [B,C,H,W] float32 pairs with H, W > 160 -> float64 [B], the channel mean of the per-channel MS-SSIM (0 for a
    channel one of whose level means is not positive).  The value-only path of `m2t_msssim_loss_tensor` (k_msssim_loss.hip);
    parity with the packages is unpinned (neither is vendored)."""
    from .losses import _msssim_call, _msssim_check
    _msssim_check("ms_ssim_device", x, y, data_range)
    _, _, per = _msssim_call(x, y, data_range, False, True)
    return per.view(x.shape[0], x.shape[1]).mean(dim=1)


def vif_device(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """``piq.vif_p(x, y, data_range=data_range, reduction='none')`` on the device: [B,C,H,W] float32 pairs with C = 1 or 3 and
    H, W >= 41 -> float64 [B], the pixel-domain VIF of the luminance planes (sigma_n_sq = 2; it exceeds 1 for a contrast-enhanced
    x).  The value-only path of `m2t_vif_loss_tensor` (k_vif_loss.hip); parity with the package is unpinned (it is not vendored)."""
    from . import _lib
    from .losses import _vif_call, _vif_check
    _vif_check("vif_device", x, y, data_range, _lib.VIF_SIGMA_N_SQ)
    _, _, per = _vif_call(x, y, data_range, _lib.VIF_SIGMA_N_SQ, False, True)
    return per


def evaluate(model, pairs, scale: int, rgb_range: float = 1.0, with_gmsd: bool = False, with_fsim: bool = False,
             with_vif: bool = False, self_ensemble: bool = False):
    """The reference's test loop (test.py:77-122): `pairs` yields (lr, hr) device tensors [1,3,h,w] / [1,3,h*scale,w*scale];
    returns (avg_psnr, avg_ssim) -- with_gmsd: + avg_gmsd; with_fsim: + avg_fsim, in the order the reference prints them
    (PSNR, SSIM, FSIM, GMSD; test.py:118-122) -- rounded as the reference rounds them; with_vif: + the average
    pixel-domain VIF of (sr, hr) at data range `rgb_range`, after everything else, rounded like FSIM / GMSD (SR sides of at least
    41).  One host synchronisation at the end (the reference synchronises per image).  self_ensemble: `model` runs on the eight flips
    and transposes of each lr and the outputs are averaged (infer.SelfEnsemble, the "+" row of a results table)."""
    if self_ensemble:
        from .infer import SelfEnsemble
        model = SelfEnsemble(model)
    rows, grows, frows, vrows = [], [], [], []
    with torch.no_grad():
        for lr, hr in pairs:
            sr = model(lr)
            if sr.shape != hr.shape:
                raise ValueError(f"hr {tuple(hr.shape)} does not match sr {tuple(sr.shape)}")
            if with_fsim:
                frows.append(fsim_device(hr, sr, 1.0))          # BEFORE the Y conversion, on RGB, like test.py:95-99
            if with_gmsd:
                grows.append(gmsd_device(hr, sr, 1.0))
            if with_vif:
                vrows.append(vif_device(sr, hr, rgb_range))
            rows.append(y_metrics_device(sr, hr, scale, rgb_range))
    if not rows:
        raise ValueError("no evaluation pairs")
    m = torch.cat(rows).cpu()
    psnr = [-10.0 * math.log10(float(v)) for v in m[:, 0]]
    avg_psnr = round(sum(psnr) / len(psnr) + 5e-3, 2)
    avg_ssim = round(float(m[:, 1].sum()) / len(psnr) + 5e-5, 4)
    out = [avg_psnr, avg_ssim]
    if with_fsim:
        out.append(round(float(torch.cat(frows).sum()) / len(psnr) + 5e-5, 4))
    if with_gmsd:
        out.append(round(float(torch.cat(grows).sum()) / len(psnr) + 5e-5, 4))
    if with_vif:
        out.append(round(float(torch.cat(vrows).sum()) / len(psnr) + 5e-5, 4))
    return tuple(out)


def lr_psnr_device(sr: torch.Tensor, lr: torch.Tensor, scale: int, rgb_range: float = 1.0) -> torch.Tensor:
    """LR-PSNR, the consistency score of the NTIRE reports: ``-10 log10(mean r^2)`` with r = (D(clamp(sr)) - lr) / rgb_range, D the
    bicubic x`scale` down-sampler; device tensors sr [B,C,H*scale,W*scale], lr [B,C,H,W] -> float64 [1] on the device (inf for an
    exactly consistent pair).  The value-only path of `m2t_consistency_loss_tensor` (k_consistency.hip): no host read."""
    from .losses import _consistency_call, _consistency_check
    _consistency_check("lr_psnr_device", sr, lr, scale, 0.0, rgb_range, lr_no_grad=False)
    _, _, stats = _consistency_call(sr, lr, scale, 0.0, rgb_range, True, False, True)
    return -10.0 * torch.log10(stats[2:3])


def evaluate_with_lr_psnr(model, pairs, scale: int, rgb_range: float = 1.0, self_ensemble: bool = False, **with_metrics):
    """`evaluate` with the average LR-PSNR of (sr, lr) appended to its outputs, rounded like PSNR; the model runs once per pair
    (`evaluate`'s own signature is pinned, so the score has an entry of its own).  The per-image values stay on the device until
    `evaluate` has made its one host synchronisation."""
    if self_ensemble:
        from .infer import SelfEnsemble
        model = SelfEnsemble(model)
    rows = []

    def scored(lr):
        sr = model(lr)
        rows.append(lr_psnr_device(sr, lr, scale, rgb_range))
        return sr
    out = evaluate(scored, pairs, scale, rgb_range, **with_metrics)
    return out + (round(float(torch.cat(rows).sum()) / len(rows) + 5e-3, 2),)
