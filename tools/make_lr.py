"""Write the bicubic LR folder of an HR folder, in the reference's layout, with the resize done on the device.

    python tools/make_lr.py --hr DIR --out DIR --scale {2,3,4} [--npy-cache DIR] [--degradation YAML]

For every image ``<name>.<ext>`` (png / jpg / jpeg / bmp) of --hr: the top-left multiple-of-scale part is resized by
m2t_imresize_u8 (MATLAB-style imresize(..., 'bicubic'), include/m2t_resize.h) and written to ``<out>/X{s}/<name>x{s}.png`` -- what
datas/us1k.py:84 and datas/benchmark.py read as ``<LR_folder>/X{s}/...``.  With --npy-cache the same array is also saved as
``<cache>/us1k_lr_x{s}/rgb/<name>x{s}.npy``, the reference's LR cache (datas/us1k.py:90-91,133-136), so that the reference's own
loaders and this library's folder path (datas.US1K(HR_folder, LR_folder, CACHE_folder)) both consume the result.  PIL does the
file I/O only.  Prints one JSON line.  Needs a device: without one it fails.  The output is always PNG: a lossy format would
re-degrade the LR image.  Consequence for a .jpg HR folder: the reference's benchmark loader and this library's
`datas.Benchmark(HR_folder, LR_folder)` look for ``<name>x{s}.jpg`` there (datas/benchmark.py:33-43; .png only when the HR path
contains "US1K_23") and do not find these files; use `datas.Benchmark(HR_folder, None)`, which synthesises the same LR images.

With --degradation the files are degraded LR images instead of bicubic ones (m2t_degrade_image_u8, include/m2t_degrade.h): YAML holds
the arguments of m2trans_amd.degrade.Degradation as a mapping (the `degradation:` mapping of a training config, on its own or
under that key); per image, in sorted file order, the blur kernel and the two noise levels are drawn from a fresh
``random.Random(seed)`` -- the images `datas.Benchmark(HR_folder, None, degradation=...)` computes for the same file order."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hr", required=True, help="folder of HR images")
    ap.add_argument("--out", required=True, help="LR folder to write (X{s}/ is created below it)")
    ap.add_argument("--scale", type=int, required=True, choices=[2, 3, 4])
    ap.add_argument("--npy-cache", default=None, help="cache folder: also write us1k_lr_x{s}/rgb/<name>x{s}.npy")
    ap.add_argument("--degradation", default=None, metavar="YAML", help="a yaml mapping of Degradation's arguments: write degraded LR "
                    "images (blur-kernel bank, speckle, noise) instead of bicubic ones")
    return ap.parse_args(argv)


def lr_paths(args, tag: str):
    """(png path, npy path or None) of one HR file name."""
    stem = os.path.splitext(tag)[0]
    s = args.scale
    png = os.path.join(args.out, f"X{s}", f"{stem}x{s}.png")
    npy = os.path.join(args.npy_cache, f"us1k_lr_x{s}", "rgb", f"{stem}x{s}.npy") if args.npy_cache else None
    return png, npy


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise SystemExit("make_lr.py needs a HIP device: the resize runs there and has no host fallback")
    from m2trans_amd.resize import imresize_u8, modcrop
    degradation = rng = None
    if args.degradation:
        import random
        import yaml
        from m2trans_amd.degrade import BENCHMARK_NOISE_ID, from_config
        with open(args.degradation) as f:
            cfg = yaml.safe_load(f) or {}
        degradation = from_config(args.scale, cfg.get("degradation", cfg) if isinstance(cfg, dict) else cfg)
        rng = random.Random(degradation.seed)
    tags = sorted(t for t in os.listdir(args.hr) if t.lower().endswith(EXTENSIONS))
    if not tags:
        raise SystemExit(f"no image in {args.hr}")
    os.makedirs(os.path.join(args.out, f"X{args.scale}"), exist_ok=True)
    if args.npy_cache:
        os.makedirs(os.path.join(args.npy_cache, f"us1k_lr_x{args.scale}", "rgb"), exist_ok=True)
    for k, tag in enumerate(tags):
        hr = modcrop(np.asarray(Image.open(os.path.join(args.hr, tag)).convert("RGB")), args.scale)
        hr_dev = torch.from_numpy(np.ascontiguousarray(hr)).cuda()
        if degradation is not None:
            index, sa, ss = degradation.draw_levels(rng)
            quality = degradation.draw_jpeg(rng) if degradation.jpeg is not None else 0     # `jpeg:` in the mapping, as datas.Benchmark
            lr = degradation.apply_image(hr_dev, index, sa, ss, BENCHMARK_NOISE_ID + k, quality=quality).cpu().numpy()
        else:
            lr = imresize_u8(hr_dev, args.scale).cpu().numpy()
        png, npy = lr_paths(args, tag)
        Image.fromarray(lr, "RGB").save(png)
        if npy:
            np.save(npy, lr)
    print(json.dumps({"images": len(tags), "scale": args.scale, "degradation": bool(args.degradation), "out": os.path.join(args.out, f"X{args.scale}"),
                      "npy_cache": os.path.join(args.npy_cache, f"us1k_lr_x{args.scale}", "rgb") if args.npy_cache else None}))


if __name__ == "__main__":
    main()
