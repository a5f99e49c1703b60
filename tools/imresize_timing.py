"""What the bicubic resampler (m2t_imresize_u8, k_resize.hip) costs: microseconds per image and bytes moved per second for down x2,
x3, x4 on an 800 x 600 HR image (W x H; mod-cropped to 798 x 600 at x3) and up x4 on 200 x 150, and the time to build the `lr_pool`
of a 1 000-image `datas.US1K` from HR alone.

Method: every case is warmed up, then timed with device events around `--reps` back-to-back launches, `--repeats` times; the
median is reported with the repeats.  Each launch of a case works on its own image of a ring of `--ring` images (source and
destination), so that the ring (ring x (in + out) bytes) is far larger than the L2 and, at the default, than the Infinity Cache:
"bytes_per_s" = (input + output bytes of one image) / time per image, the traffic the algorithm needs, not a counter.
"hbm_fraction" is that rate over the 6.3e12 B/s a streaming copy achieves on the MI355X.  One 800 x 600 image is 1.4 MB in and at
most 0.36 MB out and makes 247 workgroups at x2, 117 at x3 and 70 at x4 -- fewer than the 256 CUs --, so these are the numbers
of a short, latency-bound launch, named as such.  The pool build is a host clock around `US1K(images=[(hr, None)] * n)` ending in
a device synchronise: host concatenation, the upload and n launches.  Prints one JSON line.  Needs a device: without one it fails.

    python tools/imresize_timing.py [--reps 200] [--repeats 5] [--ring 400] [--pool-images 1000]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
CASES = (("down_x2", 2, False, 600, 800), ("down_x3", 3, False, 600, 800), ("down_x4", 4, False, 600, 800), ("up_x4", 4, True, 150, 200))
RESULT_KEYS = ("workload", "reps", "repeats", "ring", "cases", "pool_images", "pool_build_s", "pool_build_s_repeats")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="launches per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ring", type=int, default=400, help="distinct images the launches cycle through")
    ap.add_argument("--pool-images", type=int, default=1000)
    args = ap.parse_args(argv)
    if min(args.reps, args.repeats, args.ring) < 1 or args.pool_images < 0:
        ap.error("counts must be positive")
    return args


def case_bytes(scale, up, H, W):
    """Bytes one uint8 HWC image needs moved: input + output."""
    oh, ow = (H * scale, W * scale) if up else (H // scale, W // scale)
    return 3 * (H * W + oh * ow)


def case_result(scale, up, H, W, us_repeats):
    us = statistics.median(us_repeats)
    rate = case_bytes(scale, up, H, W) / (us * 1e-6)
    return {"scale": scale, "up": up, "H": H, "W": W, "us_per_image": round(us, 3), "us_repeats": [round(v, 3) for v in us_repeats],
            "bytes_per_image": case_bytes(scale, up, H, W), "bytes_per_s": round(rate, 1), "hbm_fraction": round(rate / HBM_ACHIEVABLE, 4)}


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("imresize_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.datas import US1K
    lib = _lib.load()
    st = _lib.stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(33)
    cases = {}
    for name, scale, up, H, W in CASES:
        H, W = (H, W) if up else (H - H % scale, W - W % scale)         # the mod-crop of the dataset path (800 -> 798 at x3)
        oh, ow = (H * scale, W * scale) if up else (H // scale, W // scale)
        src = torch.randint(0, 256, (args.ring, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
        dst = torch.empty(args.ring, oh, ow, 3, device="cuda", dtype=torch.uint8)
        sp, dp, sn, dn = src.data_ptr(), dst.data_ptr(), H * W * 3, oh * ow * 3

        def run(n):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for k in range(n):
                j = k % args.ring
                _lib.check(lib.m2t_imresize_u8(sp + j * sn, H, W, 3, dp + j * dn, scale, int(up), st), "m2t_imresize_u8")
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / n

        run(min(args.reps, 20))
        cases[name] = case_result(scale, up, H, W, [run(args.reps) for _ in range(args.repeats)])
        del src, dst
    pool = []
    if args.pool_images:
        rng = np.random.default_rng(33)
        images = [(rng.integers(0, 256, size=(600, 800, 3), dtype=np.uint8), None)] * args.pool_images
        for _ in range(min(3, args.repeats) + 1):                      # the first build is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = US1K(scale=4, patch_size=256, images=images)
            torch.cuda.synchronize()
            pool.append(time.perf_counter() - t0)
            del ds
        pool = pool[1:]
    out = {"workload": "MATLAB-style bicubic imresize, uint8 HWC: down x2/x3/x4 of 800x600, up x4 of 200x150; lr_pool of US1K from HR alone",
           "reps": args.reps, "repeats": args.repeats, "ring": args.ring, "cases": cases, "pool_images": args.pool_images,
           "pool_build_s": round(statistics.median(pool), 4) if pool else None, "pool_build_s_repeats": [round(v, 4) for v in pool]}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
