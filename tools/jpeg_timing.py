"""What the JPEG stage (Degradation(jpeg=(lo, hi)), m2t_degrade_jpeg_patches, include/m2t_jpeg.h) costs, at the sizes of
tools/degrade_timing.py (the configs[1] sizes of bench.py): x4, LR 128 x 128 (patch 512), batch 16, bf16, M2Trans with `--n-blocks`
blocks, on a synthetic `US1K(images=...)`.  The default Degradation: a bank of 256 kernels of 20 x 20 taps, both noises on.

"kernels_us": 16 items per call from descriptor tables built once, by device events over back-to-back calls (`--kernel-reps` per
    repeat), in alternating order:
    degrade       m2t_degrade_patches alone;
    degrade_aa    the same once more: the A/A pair.  "kernel_aa_spread" = |median(degrade) - median(degrade_aa)| / median(degrade);
    jpeg_skipped  m2t_degrade_jpeg_patches with every quality 0: the stage's LDS and arguments, none of its work;
    jpeg_on       m2t_degrade_jpeg_patches with the qualities drawn from (30, 95).
"ms_per_step": the `US1K.batch` + `TrainStep.step` loop
    off     with the Degradation without `jpeg`: the loop as it was;
    off_aa  the same once more.  "aa_spread" = |median(off) - median(off_aa)| / median(off) is what this box cannot tell apart;
    on      with `jpeg=(30, 95)`.
"stage_us" = jpeg_on - degrade, "skip_us" = jpeg_skipped - degrade (the kernels alone), "on_minus_off_ms" the loops.

Method: as tools/degrade_timing.py -- every variant is warmed up, then timed `--repeats` times, the order of the variants reversed on
every other repeat; medians are reported with the repeats.  Prints one JSON line.  Needs a device: without one it fails.

    python tools/jpeg_timing.py [--steps 20] [--repeats 5] [--n-blocks 8] [--kernel-reps 200]
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

RESULT_KEYS = ("workload", "steps", "repeats", "n_blocks", "ksize", "jpeg", "kernels_us", "kernel_aa_spread", "stage_us", "skip_us",
               "ms_per_step", "aa_spread", "on_minus_off_ms")
SCALE, LR_SIDE, BATCH = 4, 128, 16
JPEG = (30, 95)


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


def event_us(fn, n: int) -> float:
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / n


def alternate(variants: dict, measure, repeats: int) -> dict:
    for fn in variants.values():
        measure(fn, warm=True)
    out = {k: [] for k in variants}
    for r in range(repeats):
        for k in (list(variants) if r % 2 == 0 else list(reversed(variants))):
            out[k].append(measure(variants[k], warm=False))
    return out


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_timing.py needs a HIP device: nothing is measured without one")
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
    D, DJ = Degradation(SCALE), Degradation(SCALE, jpeg=JPEG)
    off, on = US1K(degradation=D, **common), US1K(degradation=DJ, **common)
    gen = torch.Generator()
    gen.manual_seed(33)

    def loop(ds):
        def run():
            idx = torch.randperm(len(ds), generator=gen).tolist()
            for i in range(0, len(idx), BATCH):
                lr, hr = ds.batch(idx[i:i + BATCH])
                ts.step(lr, hr)
        return run

    ms = alternate({"off": loop(off), "off_aa": loop(off), "on": loop(on)}, lambda fn, warm: wall_ms_per_step(fn, args.steps), args.repeats)
    med = {k: statistics.median(v) for k, v in ms.items()}

    # the kernels alone: descriptor tables built once, 16 items, the same draws behind all of them
    lib = _lib.load()
    dsc = np.zeros((BATCH, _lib.JPEG_DESC_COLS), dtype=np.int64)
    lev = np.zeros((BATCH, 2))
    for k in range(BATCH):
        _, hr_off, _, _, hr_h, hr_w = off._geo[k % 4]
        lx, ly, flags = off.draw(k)
        index, lev[k, 0], lev[k, 1], nid = DJ.draw()
        dsc[k, :8] = (hr_off, hr_h, hr_w, lx, ly, flags, index, nid)
        dsc[k, 10] = 1
        dsc[k, 11] = DJ.draw_jpeg()
    dsc[:, 8:10] = lev.view(np.int64)
    plain = np.ascontiguousarray(dsc[:, :_lib.DEGRADE_DESC_COLS])
    skipped = dsc.copy()
    skipped[:, 11] = 0
    lr = torch.empty(BATCH, 3, LR_SIDE, LR_SIDE, dtype=torch.float32, device="cuda")
    hr = torch.empty(BATCH, 3, side, side, dtype=torch.float32, device="cuda")
    bank, consts = DJ.bank_on("cuda"), DJ.jpeg_constants_on("cuda")

    def k_degrade():
        _lib.check(lib.m2t_degrade_patches(_lib.ptr(off.hr_pool), _lib.ptr(bank), len(DJ), DJ.ksize, plain.ctypes.data_as(C.c_void_p), BATCH, 3,
                                           side, SCALE, DJ.seed, _lib.ptr(lr), _lib.ptr(hr), _lib.stream_ptr()), "m2t_degrade_patches")

    def k_jpeg(table):
        def run():
            _lib.check(lib.m2t_degrade_jpeg_patches(_lib.ptr(off.hr_pool), _lib.ptr(bank), len(DJ), DJ.ksize, _lib.ptr(consts),
                                                    table.ctypes.data_as(C.c_void_p), BATCH, 3, side, SCALE, DJ.seed, _lib.ptr(lr), _lib.ptr(hr),
                                                    _lib.stream_ptr()), "m2t_degrade_jpeg_patches")
        return run

    kernels = alternate({"degrade": k_degrade, "degrade_aa": k_degrade, "jpeg_skipped": k_jpeg(skipped), "jpeg_on": k_jpeg(dsc)},
                        lambda fn, warm: event_us(fn, 10 if warm else args.kernel_reps), args.repeats)
    kmed = {k: statistics.median(v) for k, v in kernels.items()}
    out = {"workload": f"x{SCALE} LR {LR_SIDE}x{LR_SIDE} batch {BATCH} bf16", "steps": args.steps, "repeats": args.repeats,
           "n_blocks": args.n_blocks, "ksize": DJ.ksize, "jpeg": list(JPEG), "kernels_us": summarise(kernels),
           "kernel_aa_spread": round(abs(kmed["degrade"] - kmed["degrade_aa"]) / kmed["degrade"], 4),
           "stage_us": round(kmed["jpeg_on"] - kmed["degrade"], 4), "skip_us": round(kmed["jpeg_skipped"] - kmed["degrade"], 4),
           "ms_per_step": summarise(ms), "aa_spread": round(abs(med["off"] - med["off_aa"]) / med["off"], 4),
           "on_minus_off_ms": round(med["on"] - med["off"], 4)}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
