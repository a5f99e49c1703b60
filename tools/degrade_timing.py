"""What LR synthesis beyond bicubic (datas.US1K(degradation=...), m2t_degrade_patches) costs per step, at the configs[1] sizes of
bench.py: x4, LR 128 x 128 (patch 512), batch 16, bf16, M2Trans with `--n-blocks` blocks, on a synthetic `US1K(images=...)` (random
weights and images: time does not depend on them).  The default Degradation: a bank of 256 kernels of 20 x 20 taps, both noises on.

"kernels_us": m2t_degrade_patches alone against m2t_crop_patches alone, 16 items per call from a descriptor table built once, by
    device events over back-to-back calls (`--kernel-reps` per repeat).
"ms_per_step": the `US1K.batch` + `TrainStep.step` loop
    off     on the plain dataset (bicubic LR computed once at construction): the loop as it was;
    off_aa  the same once more: the A/A pair.  "aa_spread" = |median(off) - median(off_aa)| / median(off) is what this box cannot
            tell apart;
    on      on the dataset with the Degradation.
"on_minus_off_ms" against "kernel_extra_ms" (degrade - crop, the kernels alone): a loop that slows by more than the kernel's own
time plus the spread would mean a hidden synchronisation.  "kernel_share_of_step" = the degrade kernel alone / median(off).

Method: a variant is `--steps` steps from a drained device to a drained device, by the host's clock; every variant is warmed up,
then timed `--repeats` times, the order of the variants reversed on every other repeat; medians are reported with the repeats.
Prints one JSON line.  Needs a device: without one it fails.

    python tools/degrade_timing.py [--steps 20] [--repeats 5] [--n-blocks 8] [--kernel-reps 200]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESULT_KEYS = ("workload", "steps", "repeats", "n_blocks", "ksize", "kernels_us", "ms_per_step", "aa_spread", "on_minus_off_ms",
               "kernel_extra_ms", "kernel_share_of_step")
SCALE, LR_SIDE, BATCH = 4, 128, 16


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps of a variant per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=8)
    ap.add_argument("--kernel-reps", type=int, default=200, help="calls of a kernel per timed repeat")
    args = ap.parse_args(argv)
    if min(args.steps, args.repeats, args.n_blocks, args.kernel_reps) < 1:
        ap.error("counts must be positive")
    return args


def summarise(times: dict) -> dict:
    return {k: {"median": round(statistics.median(v), 4), "repeats": [round(t, 4) for t in v]} for k, v in times.items()}


def wall_ms_per_step(fn, steps: int) -> float:
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(variants: dict, steps: int, repeats: int) -> dict:
    for fn in variants.values():
        wall_ms_per_step(fn, steps)
    out = {k: [] for k in variants}
    for r in range(repeats):
        for k in (list(variants) if r % 2 == 0 else list(reversed(variants))):
            out[k].append(wall_ms_per_step(variants[k], steps))
    return out


def event_us(fn, n: int) -> float:
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / n


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("degrade_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.datas import US1K
    from m2trans_amd.degrade import Degradation
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import make_args
    torch.manual_seed(33)
    model = create_model(make_args(SCALE, args.n_blocks, "bf16")).to("cuda")
    ts = TrainStep(model, lr=1e-4, world_size=1)
    rng = np.random.RandomState(0)
    side = LR_SIDE * SCALE
    images = [(rng.randint(0, 256, size=(side + 64, side + 32, 3)).astype(np.uint8), None) for _ in range(4)]
    common = dict(images=images, scale=SCALE, patch_size=side, repeat=args.steps * BATCH // 4, device="cuda")
    D = Degradation(SCALE)
    plain, deg = US1K(**common), US1K(degradation=D, **common)
    gen = torch.Generator()
    gen.manual_seed(33)

    def loop(ds):
        def run():
            idx = torch.randperm(len(ds), generator=gen).tolist()
            for i in range(0, len(idx), BATCH):
                lr, hr = ds.batch(idx[i:i + BATCH])
                ts.step(lr, hr)
        return run

    ms = alternate({"off": loop(plain), "off_aa": loop(plain), "on": loop(deg)}, args.steps, args.repeats)
    med = {k: statistics.median(v) for k, v in ms.items()}

    # the two kernels alone: descriptor tables built once, 16 items
    lib = _lib.load()
    lp = LR_SIDE
    crop = np.zeros((BATCH, 8), dtype=np.int64)
    dsc = np.zeros((BATCH, _lib.DEGRADE_DESC_COLS), dtype=np.int64)
    lev = np.zeros((BATCH, 2))
    for k in range(BATCH):
        lr_off, hr_off, lr_h, lr_w, hr_h, hr_w = plain._geo[k % 4]
        lx, ly, flags = plain.draw(k)
        index, lev[k, 0], lev[k, 1], nid = D.draw()
        crop[k] = (lr_off, hr_off, lr_w, hr_w, lx, ly, flags, lr_h)
        dsc[k, :8] = (hr_off, hr_h, hr_w, lx, ly, flags, index, nid)
        dsc[k, 10] = 1
    dsc[:, 8:10] = lev.view(np.int64)
    lr = torch.empty(BATCH, 3, lp, lp, dtype=torch.float32, device="cuda")
    hr = torch.empty(BATCH, 3, side, side, dtype=torch.float32, device="cuda")
    bank = D.bank_on("cuda")

    def k_crop():
        _lib.check(lib.m2t_crop_patches(_lib.ptr(plain.lr_pool), _lib.ptr(plain.hr_pool), crop.ctypes.data_as(C.c_void_p), BATCH, 3, side,
                                        SCALE, _lib.ptr(lr), _lib.ptr(hr), _lib.stream_ptr()), "m2t_crop_patches")

    def k_degrade():
        _lib.check(lib.m2t_degrade_patches(_lib.ptr(deg.hr_pool), _lib.ptr(bank), len(D), D.ksize, dsc.ctypes.data_as(C.c_void_p), BATCH, 3,
                                           side, SCALE, D.seed, _lib.ptr(lr), _lib.ptr(hr), _lib.stream_ptr()), "m2t_degrade_patches")

    kernels = {"crop_patches": [], "degrade_patches": []}
    for fn in (k_crop, k_degrade):
        event_us(fn, 10)
    for r in range(args.repeats):
        for name, fn in ((("crop_patches", k_crop), ("degrade_patches", k_degrade)) if r % 2 == 0 else
                         (("degrade_patches", k_degrade), ("crop_patches", k_crop))):
            kernels[name].append(event_us(fn, args.kernel_reps))
    kmed = {k: statistics.median(v) for k, v in kernels.items()}
    out = {"workload": f"x{SCALE} LR {LR_SIDE}x{LR_SIDE} batch {BATCH} bf16", "steps": args.steps, "repeats": args.repeats,
           "n_blocks": args.n_blocks, "ksize": D.ksize, "kernels_us": summarise(kernels), "ms_per_step": summarise(ms),
           "aa_spread": round(abs(med["off"] - med["off_aa"]) / med["off"], 4), "on_minus_off_ms": round(med["on"] - med["off"], 4),
           "kernel_extra_ms": round((kmed["degrade_patches"] - kmed["crop_patches"]) * 1e-3, 4),
           "kernel_share_of_step": round(kmed["degrade_patches"] * 1e-3 / med["off"], 4)}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
