"""The inference end (include/m2t_infer.h, k_infer.hip): from a trained model and a folder of images to a folder of results, what
the reference's test.py / train.py:275-278 do with ``save_image(sr, ...)``; with geometric self-ensemble (the "+" row of an SR
results table: the model runs on the eight flips and transposes of the input as ONE batch, the outputs are mapped back and
averaged) and the per-pixel spread of the eight outputs (test-time-augmentation uncertainty).

    python -m m2trans_amd.infer --config configs/M2Trans_x4_test.yml --model_path model.pt --input LR_DIR --output SR_DIR \\
        [--self_ensemble] [--spread SPREAD_DIR] [--compute_dtype bf16|fp32] [--lean] [--local_norm T] [--tile T [--tile_overlap V] [--tile_batch N] [--seam SEAM_DIR]]

Tiled inference (include/m2t_tiles.h, k_tiles.hip; restated by tests/tiles_ref.py): the model runs on overlapping tiles of the
training size, in batches, and the outputs are feather-blended; its InstanceNorms then see the statistics they were trained with, and
every image of every size runs on one plan.

View k = 4 t + 2 v + h of a plane x[H,W]: y[i,j] = x[v ? H-1-i : i, h ? W-1-j : j], transposed when t = 1; the inverse un-transposes
first and applies the same flips; mean, spread and the 8-bit rounding are defined in include/m2t_infer.h and restated in torch by
tests/infer_ref.py.  Device tensors only: there is no host fallback.  Inference only: nothing here has a gradient."""
from __future__ import annotations

import json
import os

import torch
import torch.nn as nn

from . import _lib
from ._lib import M2TError

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def _check_planes(who: str, t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or not t.is_cuda or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise M2TError(f"{who}: {what} must be a contiguous float32 [N,C,H,W] device tensor, got {got}")


def _pack(x: torch.Tensor):
    """(a, b, whole): the views 0 .. 3 [4N,C,H,W], the views 4 .. 7 [4N,C,W,H] and, for H == W, both as one [8N,C,H,H] batch."""
    _check_planes("dihedral_pack", x, "x")
    if x.requires_grad:
        raise M2TError("dihedral_pack: inference only, x must not require a gradient")
    N, C, H, W = x.shape
    n = 4 * N * C * H * W
    buf = torch.empty(2 * n, dtype=torch.float32, device=x.device)
    a, b = buf[:n].view(4 * N, C, H, W), buf[n:].view(4 * N, C, W, H)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().m2t_dihedral_pack(_lib.ptr(x), N * C, H, W, _lib.ptr(a), _lib.ptr(b), _lib.stream_ptr()), "m2t_dihedral_pack")
    return a, b, (buf.view(8 * N, C, H, H) if H == W else None)


def dihedral_pack(x: torch.Tensor):
    """float32 [N,C,H,W] on the device -> (a [4N,C,H,W], b [4N,C,W,H]): view k of image n sits at batch index (k mod 4) N + n of a
    (k < 4) or b (k >= 4).  One launch; the source is read once."""
    a, b, _ = _pack(x)
    return a, b


def dihedral_merge(a: torch.Tensor, b: torch.Tensor, with_spread: bool = False):
    """The outputs of the views, a [4N,C,Hs,Ws] and b [4N,C,Ws,Hs] -> their mean [N,C,Hs,Ws] after the inverse maps, or
    (mean, spread) with the per-pixel standard deviation of the eight."""
    _check_planes("dihedral_merge", a, "a")
    _check_planes("dihedral_merge", b, "b")
    N4, C, Hs, Ws = a.shape
    if N4 % 4 or N4 < 4 or tuple(b.shape) != (N4, C, Ws, Hs) or b.device != a.device:
        raise M2TError(f"dihedral_merge: a [4N,C,Hs,Ws] and b [4N,C,Ws,Hs] on one device expected, got {tuple(a.shape)} and "
                       f"{tuple(b.shape)} on {a.device} and {b.device}")
    if a.requires_grad or b.requires_grad:
        raise M2TError("dihedral_merge: inference only, the inputs must not require a gradient")
    N = N4 // 4
    mean = torch.empty(N, C, Hs, Ws, dtype=torch.float32, device=a.device)
    spread = torch.empty_like(mean) if with_spread else None
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().m2t_dihedral_merge(_lib.ptr(a), _lib.ptr(b), N * C, Hs, Ws, _lib.ptr(mean), _lib.ptr(spread),
                                                  _lib.stream_ptr()), "m2t_dihedral_merge")
    return (mean, spread) if with_spread else mean


def _model_output(out, n: int, h: int, w: int, scale=None, who: str = "self_ensemble"):
    """The scale of a model output [n,3,s h,s w] (contiguous float32 on the device), checked against `scale` when given."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 4 or not out.is_cuda or not out.is_contiguous():
        raise M2TError(f"{who}: the model must return a contiguous float32 [n,3,s*h,s*w] device tensor")
    s = out.shape[2] // h if scale is None else scale
    if s < 1 or tuple(out.shape) != (n, 3, s * h, s * w):
        raise M2TError(f"{who}: model output {tuple(out.shape)} for an input [{n},3,{h},{w}]"
                       + (" is not that input times an integer scale" if scale is None else f" does not match the scale {scale} of the first call"))
    return s


def self_ensemble(model, lr: torch.Tensor, with_spread: bool = False):
    """Geometric self-ensemble: `model` (any callable [n,3,h,w] -> contiguous float32 [n,3,s h,s w] on the device) on the eight views
    of lr [B,3,H,W], mapped back and averaged -> sr [B,3,s H,s W], or (sr, spread).  H == W: ONE call on [8B,3,H,H]; otherwise two,
    [4B,3,H,W] then [4B,3,W,H]."""
    _check_planes("self_ensemble", lr, "lr")
    if lr.shape[1] != 3:
        raise M2TError(f"self_ensemble: lr must be [B,3,H,W], got {tuple(lr.shape)}")
    if lr.requires_grad:
        raise M2TError("self_ensemble: inference only, lr must not require a gradient")
    B, _, H, W = lr.shape
    with torch.no_grad():
        a, b, whole = _pack(lr)
        if whole is not None:
            out = model(whole)
            _model_output(out, 8 * B, H, H)
            sa, sb = out[:4 * B], out[4 * B:]
        else:
            sa = model(a)
            s = _model_output(sa, 4 * B, H, W)
            sb = model(b)
            _model_output(sb, 4 * B, W, H, scale=s)
        return dihedral_merge(sa, sb, with_spread)


_self_ensemble = self_ensemble


class SelfEnsemble(nn.Module):
    """`self_ensemble` as a module around `model`: drops into `metrics.evaluate` and into the reference's test loop."""

    def __init__(self, model, with_spread: bool = False):
        super().__init__()
        self.model, self.with_spread = model, bool(with_spread)

    def forward(self, lr):
        return self_ensemble(self.model, lr, self.with_spread)


# ------------------------------------------------------------------------------------------------------------------------- tiles
def tile_grid(L: int, T: int, overlap: int):
    """The tile grid of one axis (m2t_tile_grid, the one definition the kernels use too): LR length L, tile size T, overlap with
    0 <= 2 overlap <= T -> (tile_len, origins).  L <= T: one tile of length L; otherwise tiles of length T every T - overlap, the last
    one shifted back to end at L.  Host only."""
    import ctypes as C
    lib = _lib.load()
    n, t = C.c_int(0), C.c_int(0)
    _lib.check(lib.m2t_tile_grid(int(L), int(T), int(overlap), C.byref(n), C.byref(t), None), "m2t_tile_grid")
    origins = (C.c_int * n.value)()
    _lib.check(lib.m2t_tile_grid(int(L), int(T), int(overlap), C.byref(n), C.byref(t), origins), "m2t_tile_grid")
    return t.value, list(origins)


def tile_gather(x: torch.Tensor, tile: int, overlap: int, first: int = 0, count=None) -> torch.Tensor:
    """float32 [B,C,H,W] on the device -> the tiles first .. first + count - 1 of the global order (tile (b, ky, kx) has the index
    (b ny + ky) nx + kx) as one batch [count,C,th,tw]; count = None: all from `first` on.  One launch."""
    _check_planes("tile_gather", x, "x")
    if x.requires_grad:
        raise M2TError("tile_gather: inference only, x must not require a gradient")
    B, C, H, W = x.shape
    (th, oy), (tw, ox) = tile_grid(H, tile, overlap), tile_grid(W, tile, overlap)
    total = B * len(oy) * len(ox)
    count = total - int(first) if count is None else int(count)
    if first < 0 or count < 1 or first + count > total:
        raise M2TError(f"tile_gather: tiles {first} .. {first + count - 1} asked for, the batch has {total}")
    dst = torch.empty(count, C, th, tw, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().m2t_tile_gather(_lib.ptr(x), B, C, H, W, int(tile), int(overlap), int(first), count, _lib.ptr(dst),
                                               _lib.stream_ptr()), "m2t_tile_gather")
    return dst


def tile_blend(tiles: torch.Tensor, B: int, H: int, W: int, tile: int, overlap: int, scale: int, with_seam: bool = False):
    """The outputs of all tiles of a batch [B,C,H,W], tiles [B ny nx,C,s th,s tw] in the global order -> the feather-blended image
    [B,C,s H,s W], or (image, seam) with the weighted standard deviation of the covering tiles per element (0 where one tile covers).
    The weights, the order of the sums and the single-cover copy are defined in include/m2t_tiles.h.  One launch."""
    _check_planes("tile_blend", tiles, "tiles")
    if tiles.requires_grad:
        raise M2TError("tile_blend: inference only, the tiles must not require a gradient")
    (th, oy), (tw, ox) = tile_grid(H, tile, overlap), tile_grid(W, tile, overlap)
    s, C = int(scale), tiles.shape[1]
    want = (int(B) * len(oy) * len(ox), C, s * th, s * tw)
    if B < 1 or tuple(tiles.shape) != want:
        raise M2TError(f"tile_blend: tiles {tuple(tiles.shape)}, expected {want} for B = {B}, an image {H} x {W}, tile {tile}, overlap "
                       f"{overlap} and scale {scale}")
    out = torch.empty(B, C, s * H, s * W, dtype=torch.float32, device=tiles.device)
    seam = torch.empty_like(out) if with_seam else None
    with torch.cuda.device(tiles.device):
        _lib.check(_lib.load().m2t_tile_blend(_lib.ptr(tiles), int(B), C, int(H), int(W), int(tile), int(overlap), s, _lib.ptr(out),
                                              _lib.ptr(seam), _lib.stream_ptr()), "m2t_tile_blend")
    return (out, seam) if with_seam else out


def tiled(model, lr: torch.Tensor, tile: int = 128, overlap: int = 16, tile_batch: int = 16, with_seam: bool = False):
    """`model` (any callable under the contract of `self_ensemble`) on overlapping tiles of lr [B,3,H,W], the outputs feather-blended
    -> sr [B,3,s H,s W], or (sr, seam).  The tiles are gathered and run in chunks of `tile_batch` (every chunk on the one
    (tile_batch, tile, tile) plan, the last chunk on a smaller one), each chunk's output is copied into one SR-tile buffer, one blend
    follows.  When both axes have a single tile the result is `model(lr)` itself and nothing else is launched (a seam is then all 0).
    A model that returns several tensors of the SR shape, as `SelfEnsemble(model, with_spread=True)` does, has each of them blended
    with the same weights: (sr, spread) or (sr, spread, seam), the seam being that of the first.  A tile that is not a multiple of 32
    makes the model reflect-pad every tile."""
    _check_planes("tiled", lr, "lr")
    if lr.shape[1] != 3:
        raise M2TError(f"tiled: lr must be [B,3,H,W], got {tuple(lr.shape)}")
    if lr.requires_grad:
        raise M2TError("tiled: inference only, lr must not require a gradient")
    tile_batch = int(tile_batch)
    if tile_batch < 1:
        raise M2TError(f"tiled: tile_batch must be positive, got {tile_batch}")
    B, _, H, W = lr.shape
    (th, oy), (tw, ox) = tile_grid(H, tile, overlap), tile_grid(W, tile, overlap)
    total = B * len(oy) * len(ox)
    with torch.no_grad():
        if len(oy) == 1 and len(ox) == 1:
            out = model(lr)
            if not with_seam:
                return out
            outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
            _model_output(outs[0], B, H, W, who="tiled")
            return outs + (torch.zeros_like(outs[0]),)
        s, bufs = None, None
        for first in range(0, total, tile_batch):
            count = min(tile_batch, total - first)
            out = model(tile_gather(lr, tile, overlap, first, count))
            outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
            for o in outs:
                s = _model_output(o, count, th, tw, scale=s, who="tiled")
            if bufs is None:
                bufs = [torch.empty(total, 3, s * th, s * tw, dtype=torch.float32, device=lr.device) for _ in outs]
            elif len(bufs) != len(outs):
                raise M2TError(f"tiled: the model returned {len(outs)} tensors for one chunk and {len(bufs)} for the first")
            for buf, o in zip(bufs, outs):
                buf[first:first + count].copy_(o)
        res = [tile_blend(buf, B, H, W, tile, overlap, s) for buf in bufs[1:]]
        head = tile_blend(bufs[0], B, H, W, tile, overlap, s, with_seam)
        if with_seam:
            return (head[0], *res, head[1])
        return (head, *res) if res else head


class Tiled(nn.Module):
    """`tiled` as a module around `model`: drops into `metrics.evaluate`, and composes with `SelfEnsemble`:
    `Tiled(SelfEnsemble(model))` ensembles per tile (square tiles: ONE model call on 8 * tile_batch views per chunk)."""

    def __init__(self, model, tile: int = 128, overlap: int = 16, tile_batch: int = 16, with_seam: bool = False):
        super().__init__()
        self.model, self.tile, self.overlap, self.tile_batch, self.with_seam = model, int(tile), int(overlap), int(tile_batch), bool(with_seam)

    def forward(self, lr):
        return tiled(self.model, lr, self.tile, self.overlap, self.tile_batch, self.with_seam)


def back_project(sr: torch.Tensor, lr: torch.Tensor, scale: int, iters: int = 3, beta: float = 1.0, rgb_range: float = 1.0,
                 with_stats: bool = False):
    """Irani-Peleg back-projection towards LR-consistency: `iters` times ``sr <- clamp(sr + beta * U(lr - D(clamp(sr))), 0,
    rgb_range)``, D / U the bicubic x`scale` down- / up-sampler of `resize.imresize` (m2t_back_project_f32 of
    include/m2t_consistency.h: the residual in fp64, one fp32 rounding per updated pixel).  Device tensors sr [B,C,H*scale,W*scale] and
    lr [B,C,H,W], C = 1 or 3, 0 < beta < 2; returns a NEW tensor.  with_stats: also a float64 device tensor [iters + 1, 3], row k =
    {mean |r|, max |r|, mean r^2} of r = (lr - D(clamp(sr_k))) / rgb_range before update k, the last row taken after the last update
    (LR-PSNR = -10 log10 of the third column).  No host read."""
    from .losses import _consistency_check
    _consistency_check("back_project", sr, lr, scale, 0.0, rgb_range, lr_no_grad=False)
    iters = int(iters)
    if iters < 0:
        raise M2TError(f"back_project: iters must be >= 0, got {iters}")
    import math
    if not (math.isfinite(float(beta)) and 0.0 < float(beta) < 2.0):
        raise M2TError(f"back_project: beta must be a finite number inside (0, 2), got {beta!r}")
    lib = _lib.load()
    out = sr.detach().float().clone(memory_format=torch.contiguous_format)
    yc = lr.detach().contiguous().float()
    B, Cn, H, W = yc.shape
    nbytes = lib.m2t_consistency_scratch_bytes(B, Cn, H, W, int(scale))
    if nbytes == 0:
        raise M2TError(f"back_project: no scratch size for LR [{B},{Cn},{H},{W}] x{scale} (SR sides at most 16384, B * C at most 65535)")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
    stats = torch.empty(iters + 1, 3, dtype=torch.float64, device=out.device) if with_stats else None
    with torch.cuda.device(out.device):
        st = _lib.stream_ptr()
        for k in range(iters + (1 if with_stats else 0)):
            _lib.check(lib.m2t_back_project_f32(_lib.ptr(out), _lib.ptr(yc), B, Cn, H, W, int(scale), float(rgb_range), float(beta),
                                                int(k < iters), _lib.ptr(stats[k]) if with_stats else None, _lib.ptr(scratch), st),
                       "m2t_back_project_f32")
    return (out, stats) if with_stats else out


class BackProject(nn.Module):
    """`back_project` as a module around `model` (``lr -> sr``): composes OUTSIDE `Tiled` / `SelfEnsemble`
    (``BackProject(Tiled(SelfEnsemble(model)), 4)``: consistency is a property of the whole image) and drops into `metrics.evaluate`."""

    def __init__(self, model, scale: int, iters: int = 3, beta: float = 1.0, rgb_range: float = 1.0):
        super().__init__()
        self.model, self.scale, self.iters, self.beta, self.rgb_range = model, int(scale), int(iters), float(beta), float(rgb_range)

    def forward(self, lr):
        return back_project(self.model(lr), lr, self.scale, self.iters, self.beta, self.rgb_range)


def to_uint8(sr: torch.Tensor, rgb_range: float = 1.0) -> torch.Tensor:
    """float32 [1,C,H,W] or [C,H,W] on the device, C = 1 or 3 -> uint8 [H,W,C] on the device with the rounding of torchvision's
    save_image: min(max(v * (255 / rgb_range) + 0.5, 0), 255) truncated; a NaN becomes 0."""
    if isinstance(sr, torch.Tensor) and sr.dim() == 4 and sr.shape[0] == 1:
        sr = sr[0]
    if not isinstance(sr, torch.Tensor) or sr.dtype != torch.float32 or sr.dim() != 3 or not sr.is_cuda:
        got = f"{sr.dtype} {tuple(sr.shape)} on {sr.device}" if isinstance(sr, torch.Tensor) else type(sr).__name__
        raise M2TError(f"to_uint8 takes a float32 [1,C,H,W] or [C,H,W] device tensor, got {got}")
    sr = sr.detach().contiguous()
    C, H, W = sr.shape
    out = torch.empty(H, W, C, dtype=torch.uint8, device=sr.device)
    with torch.cuda.device(sr.device):
        _lib.check(_lib.load().m2t_tensor_to_image_u8(_lib.ptr(sr), C, H, W, float(rgb_range), _lib.ptr(out), _lib.stream_ptr()),
                   "m2t_tensor_to_image_u8")
    return out


def save_image(sr: torch.Tensor, path, rgb_range: float = 1.0) -> None:
    """Write [1,C,H,W] or [C,H,W] (C = 3: RGB, C = 1: grey) as an 8-bit image through PIL; the format follows the file name."""
    from PIL import Image
    img = to_uint8(sr, rgb_range).cpu().numpy()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(str(path))


def image_names(in_dir) -> list:
    """The image files of a folder, sorted by name."""
    return sorted(f for f in os.listdir(str(in_dir)) if f.lower().endswith(IMAGE_EXTENSIONS))


def output_name(name: str) -> str:
    """`<name>.<ext>` of the input folder -> `<name>.png` of the output folder."""
    return os.path.splitext(os.path.basename(name))[0] + ".png"


def output_names(names) -> list:
    out = [output_name(n) for n in names]
    if len(set(out)) != len(out):
        dup = sorted({n for n in out if out.count(n) > 1})
        raise M2TError(f"input files that differ only in their extension would be written to the same file: {dup}")
    return out


def load_image(path, device, rgb_range: float = 1.0) -> torch.Tensor:
    """An image file as PIL ``convert("RGB")`` -> float32 [1,3,H,W] in [0, rgb_range] on the device (m2t_image_to_tensor)."""
    import numpy as np
    from PIL import Image
    u8 = torch.from_numpy(np.array(Image.open(str(path)).convert("RGB"))).to(device)
    H, W = u8.shape[0], u8.shape[1]
    lr = torch.empty(1, 3, H, W, dtype=torch.float32, device=u8.device)
    with torch.cuda.device(u8.device):
        _lib.check(_lib.load().m2t_image_to_tensor(_lib.ptr(u8), H, W, 3, H, W, _lib.ptr(lr), _lib.stream_ptr()), "m2t_image_to_tensor")
    return lr if rgb_range == 1.0 else lr * float(rgb_range)


def _save_map(grey_of: torch.Tensor, path) -> float:
    """A per-element map [1,3,H,W] as an 8-bit grey PNG: its maximum over RGB, scaled by the image's own maximum; returns that maximum."""
    grey = grey_of[0].amax(dim=0, keepdim=True)
    top = float(grey.max())
    save_image(grey, path, top if top > 0.0 else 1.0)
    return top


def upscale_folder(model, in_dir, out_dir, self_ensemble: bool = False, spread_dir=None, rgb_range: float = 1.0,
                   device="cuda", tile=None, overlap: int = 16, tile_batch=None, seam_dir=None, back_project_iters: int = 0,
                   back_project_beta: float = 1.0, lean: bool = False, local_norm=None) -> list:
    """Every image of `in_dir` through `model` into `out_dir` as `<name>.png`; returns the written names.  self_ensemble: through
    the eight views.  spread_dir (needs self_ensemble): the per-pixel maximum over RGB of the spread as an 8-bit grey PNG of the same
    name, scaled by the image's own maximum (grey 255 = that maximum); `spread.json` beside the files maps each name to that maximum,
    in units of `rgb_range`.  tile: through `tiled` with that tile size, `overlap` and `tile_batch` (None: 16, or 2 with
    self_ensemble, which makes 16 views per call); the ensemble is then taken per tile.  seam_dir (needs tile): the seam map, written
    like the spread, with `seam.json`.  back_project_iters > 0: every output goes through that many iterations of `back_project` (step
    `back_project_beta`) against its own input before it is written, and `consistency.json` beside the results holds, per image,
    the mean / max residual and the LR-PSNR before and after.  lean: the model runs on inference plans for the length of this call
    (`M2Trans.lean_inference`: the same bits on a forward-only workspace); False leaves the model's own setting alone.  local_norm=T:
    for the length of this call the model normalises with the statistics of a T x T window around every pixel (`M2Trans.local_norm`,
    which implies lean); None leaves the model's own setting alone."""
    if local_norm is not None:
        was = (int(getattr(model, "local_norm_window", 0)), bool(getattr(model, "lean_inference_enabled", False)))
        model.local_norm(local_norm)
        try:
            return upscale_folder(model, in_dir, out_dir, self_ensemble, spread_dir, rgb_range, device, tile, overlap, tile_batch, seam_dir,
                                  back_project_iters, back_project_beta, lean=lean)
        finally:
            model.local_norm(was[0])
            model.lean_inference(was[1])
    if lean:
        was = bool(getattr(model, "lean_inference_enabled", False))
        model.lean_inference(True)
        try:
            return upscale_folder(model, in_dir, out_dir, self_ensemble, spread_dir, rgb_range, device, tile, overlap, tile_batch, seam_dir,
                                  back_project_iters, back_project_beta, lean=False)
        finally:
            model.lean_inference(was)
    if spread_dir is not None and not self_ensemble:
        raise M2TError("upscale_folder: spread_dir needs self_ensemble=True (the spread is that of the eight views)")
    if seam_dir is not None and tile is None:
        raise M2TError("upscale_folder: seam_dir needs a tile size (the seam is the disagreement of overlapping tiles)")
    names = image_names(in_dir)
    if not names:
        raise M2TError(f"upscale_folder: no image file in {in_dir}")
    outs = output_names(names)
    os.makedirs(str(out_dir), exist_ok=True)
    if spread_dir is not None:
        os.makedirs(str(spread_dir), exist_ok=True)
    if seam_dir is not None:
        os.makedirs(str(seam_dir), exist_ok=True)
    run = _self_ensemble                                        # (the keyword of this function shadows the module's function)
    factors, seams, cons = {}, {}, {}
    with torch.no_grad():
        for name, out in zip(names, outs):
            lr = load_image(os.path.join(str(in_dir), name), device, rgb_range)
            if tile is not None:
                inner = SelfEnsemble(model, with_spread=spread_dir is not None) if self_ensemble else model
                got = tiled(inner, lr, tile, overlap, (2 if self_ensemble else 16) if tile_batch is None else tile_batch,
                            with_seam=seam_dir is not None)
                got = list(got) if isinstance(got, (tuple, list)) else [got]
                sr = got.pop(0)
                if spread_dir is not None:
                    factors[out] = _save_map(got.pop(0), os.path.join(str(spread_dir), out))
                if seam_dir is not None:
                    seams[out] = _save_map(got.pop(0), os.path.join(str(seam_dir), out))
            elif not self_ensemble:
                sr = model(lr)
            elif spread_dir is None:
                sr = run(model, lr)
            else:
                sr, spread = run(model, lr, with_spread=True)
                factors[out] = _save_map(spread, os.path.join(str(spread_dir), out))
            if back_project_iters > 0:
                sr, cons[out] = back_project(sr, lr, sr.shape[2] // lr.shape[2], back_project_iters, back_project_beta, rgb_range,
                                             with_stats=True)
            save_image(sr, os.path.join(str(out_dir), out), rgb_range)
    if spread_dir is not None:
        with open(os.path.join(str(spread_dir), "spread.json"), "w") as f:
            json.dump({"rgb_range": float(rgb_range), "max_spread": factors}, f, indent=1, sort_keys=True)
    if seam_dir is not None:
        with open(os.path.join(str(seam_dir), "seam.json"), "w") as f:
            json.dump({"rgb_range": float(rgb_range), "max_seam": seams}, f, indent=1, sort_keys=True)
    if back_project_iters > 0:
        with open(os.path.join(str(out_dir), "consistency.json"), "w") as f:
            json.dump({"rgb_range": float(rgb_range), "iters": int(back_project_iters), "beta": float(back_project_beta),
                       "images": {n: consistency_record(t.cpu()) for n, t in cons.items()}}, f, indent=1, sort_keys=True)
    return outs


def consistency_record(stats: torch.Tensor) -> dict:
    """The first and the last row of `back_project`'s statistics (host tensor [iters + 1, 3]) as the entry of consistency.json."""
    import math

    def row(r):
        mse = float(r[2])
        return {"mean_residual": float(r[0]), "max_residual": float(r[1]), "lr_psnr": -10.0 * math.log10(mse) if mse > 0.0 else float("inf")}
    return {"before": row(stats[0]), "after": row(stats[-1])}


# ------------------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m m2trans_amd.infer", description="Super-resolve a folder of images with a trained M2Trans.")
    ap.add_argument("--config", required=True, help="the yaml the model was trained with (scale, n_blocks, n_feats, colors, rgb_range)")
    ap.add_argument("--model_path", required=True, help="a checkpoint of train.py (model_state_dict) or a bare state_dict")
    ap.add_argument("--input", required=True, help="folder of LR images")
    ap.add_argument("--output", required=True, help="folder the results are written to, as <name>.png")
    ap.add_argument("--self_ensemble", action="store_true", help="average over the eight flips and transposes of the input")
    ap.add_argument("--spread", default=None, metavar="DIR", help="with --self_ensemble: write the per-pixel spread of the eight outputs there")
    ap.add_argument("--compute_dtype", choices=("bf16", "fp32"), default=None, help="overrides the yaml's compute_dtype")
    ap.add_argument("--lean", action="store_true", help="run on inference plans: the same bits on a forward-only workspace (a fraction "
                    "of the training workspace; whole frames fit where they needed --tile before)")
    ap.add_argument("--local_norm", type=int, default=None, metavar="T", help="normalise every pixel with the InstanceNorm statistics of the "
                    "T x T window around it (8 .. 16384; the training LR patch size) instead of the whole frame's: one pass, no tiles "
                    "(implies --lean)")
    ap.add_argument("--tile", type=int, default=None, metavar="T", help="run the model on overlapping T x T tiles (the training LR patch "
                    "size, a multiple of 32) and feather-blend the outputs")
    ap.add_argument("--tile_overlap", type=int, default=16, metavar="V", help="with --tile: LR pixels two neighbouring tiles share, 0 <= 2 V <= T")
    ap.add_argument("--tile_batch", type=int, default=None, metavar="N", help="with --tile: tiles per model call (default 16, or 2 with "
                    "--self_ensemble: 16 views per call)")
    ap.add_argument("--seam", default=None, metavar="DIR", help="with --tile: write the per-pixel disagreement of overlapping tiles there")
    ap.add_argument("--back_project", type=int, default=None, metavar="K", help="K iterations of back-projection on every output against "
                    "its input (LR-consistency); writes consistency.json beside the results")
    ap.add_argument("--back_project_beta", type=float, default=None, metavar="B", help="with --back_project: the step, 0 < B < 2 (default 1)")
    args = ap.parse_args(argv)
    if args.back_project_beta is not None and args.back_project is None:
        ap.error("--back_project_beta needs --back_project")
    if args.back_project is not None:
        if args.back_project < 1:
            ap.error("--back_project must be at least 1")
        if args.back_project_beta is None:
            args.back_project_beta = 1.0
        elif not (0.0 < args.back_project_beta < 2.0):
            ap.error("--back_project_beta must lie inside (0, 2)")
    if args.spread is not None and not args.self_ensemble:
        ap.error("--spread needs --self_ensemble")
    if args.local_norm is not None and not 8 <= args.local_norm <= 16384:
        ap.error("--local_norm must lie in 8 .. 16384")
    if args.seam is not None and args.tile is None:
        ap.error("--seam needs --tile")
    if args.tile is not None:
        if args.tile < 1 or args.tile_overlap < 0 or 2 * args.tile_overlap > args.tile:
            ap.error("--tile must be positive and --tile_overlap must satisfy 0 <= 2 V <= T")
        if args.tile_batch is None:
            args.tile_batch = 2 if args.self_ensemble else 16
        elif args.tile_batch < 1:
            ap.error("--tile_batch must be positive")
    return args


def model_namespace(cfg: dict, compute_dtype=None):
    """The argparse namespace updated with the yaml dictionary, as train.py:28-34 builds it."""
    import types
    ns = types.SimpleNamespace(**dict(cfg))
    if compute_dtype is not None:
        ns.compute_dtype = compute_dtype
    return ns


def load_weights(model, ckpt) -> None:
    """A checkpoint of train.py (``model_state_dict`` inside) through `checkpoint.import_checkpoint`, a bare state_dict through
    `load_state_dict`; either with or without DataParallel's ``module.`` prefix."""
    if isinstance(ckpt, dict) and "model_state_dict" in ckpt:
        from .checkpoint import import_checkpoint
        import_checkpoint(ckpt, model)
    else:
        model.load_state_dict(ckpt, strict=True)


def main(argv=None) -> int:
    args = parse_args(argv)
    import yaml
    from .M2Trans_network import create_model
    with open(args.config) as f:
        cfg = yaml.load(f, Loader=yaml.FullLoader)
    ns = model_namespace(cfg, args.compute_dtype)
    if not torch.cuda.is_available():
        raise M2TError("python -m m2trans_amd.infer needs a HIP device: there is no host fallback")
    model = create_model(ns).to("cuda")
    load_weights(model, torch.load(args.model_path, map_location="cpu", weights_only=False))
    model.eval()
    outs = upscale_folder(model, args.input, args.output, self_ensemble=args.self_ensemble, spread_dir=args.spread,
                          rgb_range=float(getattr(ns, "rgb_range", 1.0)), tile=args.tile, overlap=args.tile_overlap,
                          tile_batch=args.tile_batch, seam_dir=args.seam, back_project_iters=args.back_project or 0,
                          back_project_beta=args.back_project_beta or 1.0, lean=args.lean, local_norm=args.local_norm)
    line = {"images": len(outs), "output": args.output, "self_ensemble": bool(args.self_ensemble), "spread": args.spread, "lean": bool(args.lean or args.local_norm),
            "local_norm": args.local_norm,
            "tile": args.tile, "tile_overlap": args.tile_overlap if args.tile is not None else None, "seam": args.seam}
    if args.back_project is not None:
        line.update({"back_project": args.back_project, "back_project_beta": args.back_project_beta,
                     "consistency": os.path.join(args.output, "consistency.json")})
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
