"""The inference end (include/m2t_infer.h, k_infer.hip): from a trained model and a folder of images to a folder of results, what
the reference's test.py / train.py:275-278 do with ``save_image(sr, ...)``; with geometric self-ensemble (the "+" row of an SR
results table: the model runs on the eight flips and transposes of the input as ONE batch, the outputs are mapped back and
averaged) and the per-pixel spread of the eight outputs (test-time-augmentation uncertainty).

    python -m m2trans_amd.infer --config configs/M2Trans_x4_test.yml --model_path model.pt --input LR_DIR --output SR_DIR \\
        [--self_ensemble] [--spread SPREAD_DIR] [--compute_dtype bf16|fp32]

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


def _model_output(out, n: int, h: int, w: int, scale=None):
    """The scale of a model output [n,3,s h,s w] (contiguous float32 on the device), checked against `scale` when given."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 4 or not out.is_cuda or not out.is_contiguous():
        raise M2TError("self_ensemble: the model must return a contiguous float32 [n,3,s*h,s*w] device tensor")
    s = out.shape[2] // h if scale is None else scale
    if s < 1 or tuple(out.shape) != (n, 3, s * h, s * w):
        raise M2TError(f"self_ensemble: model output {tuple(out.shape)} for an input [{n},3,{h},{w}]"
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


def upscale_folder(model, in_dir, out_dir, self_ensemble: bool = False, spread_dir=None, rgb_range: float = 1.0,
                   device="cuda") -> list:
    """Every image of `in_dir` through `model` into `out_dir` as `<name>.png`; returns the written names.  self_ensemble: through
    the eight views.  spread_dir (needs self_ensemble): the per-pixel maximum over RGB of the spread as an 8-bit grey PNG of the same
    name, scaled by the image's own maximum (grey 255 = that maximum); `spread.json` beside the files maps each name to that maximum,
    in units of `rgb_range`."""
    if spread_dir is not None and not self_ensemble:
        raise M2TError("upscale_folder: spread_dir needs self_ensemble=True (the spread is that of the eight views)")
    names = image_names(in_dir)
    if not names:
        raise M2TError(f"upscale_folder: no image file in {in_dir}")
    outs = output_names(names)
    os.makedirs(str(out_dir), exist_ok=True)
    if spread_dir is not None:
        os.makedirs(str(spread_dir), exist_ok=True)
    run = _self_ensemble                                        # (the keyword of this function shadows the module's function)
    factors = {}
    with torch.no_grad():
        for name, out in zip(names, outs):
            lr = load_image(os.path.join(str(in_dir), name), device, rgb_range)
            if not self_ensemble:
                sr = model(lr)
            elif spread_dir is None:
                sr = run(model, lr)
            else:
                sr, spread = run(model, lr, with_spread=True)
                grey = spread[0].amax(dim=0, keepdim=True)
                top = float(grey.max())
                save_image(grey, os.path.join(str(spread_dir), out), top if top > 0.0 else 1.0)
                factors[out] = top
            save_image(sr, os.path.join(str(out_dir), out), rgb_range)
    if spread_dir is not None:
        with open(os.path.join(str(spread_dir), "spread.json"), "w") as f:
            json.dump({"rgb_range": float(rgb_range), "max_spread": factors}, f, indent=1, sort_keys=True)
    return outs


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
    args = ap.parse_args(argv)
    if args.spread is not None and not args.self_ensemble:
        ap.error("--spread needs --self_ensemble")
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
                          rgb_range=float(getattr(ns, "rgb_range", 1.0)))
    print(json.dumps({"images": len(outs), "output": args.output, "self_ensemble": bool(args.self_ensemble), "spread": args.spread}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
