"""What the epoch loop of m2trans_amd/train.py costs per step on top of `TrainStep.step`, at the configs[1] sizes of bench.py: x4,
LR 128 x 128, batch 16, bf16, M2Trans with `--n-blocks` blocks, on a synthetic `US1K(images=...)` (random weights and images: time
does not depend on them).

    a     a bare loop of `US1K.batch` + `TrainStep.step`: what a user had to write before `fit` existed;
    b     the same loop with `float(ts.loss)` after every step: the reference's habit (train.py:212-214 reads three values);
    c     the batch loop of `fit` (train.run_epoch): loader, step, one m2t_meter_update per step; augmentation off, no log point and
          no preview inside the timed interval;
    c_aa  c once more: the A/A pair.  "aa_spread" = |median(c) - median(c_aa)| / median(c) is what this box cannot tell apart; a
          difference between two variants below it is no difference;
    d     c with `preview_every=1`: a batch-1 forward, m2t_preview_strip, the copy of the strip to the host and the PNG encoding
          after every step -- the price of a preview, not a setting anyone trains with.
"kernels": m2t_meter_update (4 columns) and m2t_preview_strip (LR 128 x 128, x4) alone, by device events over back-to-back launches.

Method: a variant is `--steps` steps from a drained device to a drained device, by the host's clock (the question is whether the
host keeps running ahead of the device, so device events around the kernels would not see it); every variant is warmed up, then
timed `--repeats` times, the order of the variants reversed on every other repeat; medians are reported with the repeats.  Prints
one JSON line.  Needs a device: without one it fails.

    python tools/train_loop_timing.py [--steps 20] [--repeats 5] [--n-blocks 8] [--kernel-reps 200]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESULT_KEYS = ("workload", "steps", "repeats", "n_blocks", "ms_per_step", "aa_spread", "c_minus_a", "kernels_us")
SCALE, LR_SIDE, BATCH = 4, 128, 16


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps of a variant per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=8)
    ap.add_argument("--kernel-reps", type=int, default=200, help="launches of a kernel per timed repeat")
    args = ap.parse_args(argv)
    if min(args.steps, args.repeats, args.n_blocks, args.kernel_reps) < 1:
        ap.error("counts must be positive")
    return args


def summarise(times: dict) -> dict:
    return {k: {"median": round(statistics.median(v), 4), "repeats": [round(t, 4) for t in v]} for k, v in times.items()}


def wall_ms_per_step(fn, steps: int) -> float:
    """fn() runs `steps` steps; milliseconds per step from a drained device to a drained device, by the host's clock."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(variants: dict, steps: int, repeats: int) -> dict:
    """{name: [ms per step, one per repeat]}; the order of the variants is reversed on every other repeat."""
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
        raise SystemExit("train_loop_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import train as T
    from m2trans_amd.datas import US1K
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import make_args
    torch.manual_seed(33)
    model = create_model(make_args(SCALE, args.n_blocks, "bf16")).to("cuda")
    ts = TrainStep(model, lr=1e-4, world_size=1)
    rng = np.random.RandomState(0)
    side = LR_SIDE * SCALE
    images = [(rng.randint(0, 256, size=(side + 64, side + 32, 3)).astype(np.uint8), None) for _ in range(4)]
    ds = US1K(images=images, scale=SCALE, patch_size=side, repeat=args.steps * BATCH // 4, device="cuda")
    assert len(ds) == args.steps * BATCH
    gen = torch.Generator()
    gen.manual_seed(33)
    names = T.meter_columns(ts)
    meter = T.StepMeter(names, "cuda")
    folder = tempfile.mkdtemp(prefix="train_loop_timing_")

    def order():
        return torch.randperm(len(ds), generator=gen).tolist()

    def a_bare():
        idx = order()
        for i in range(0, len(idx), BATCH):
            lr, hr = ds.batch(idx[i:i + BATCH])
            ts.step(lr, hr)

    def b_float_every_step():
        idx = order()
        total = 0.0
        for i in range(0, len(idx), BATCH):
            lr, hr = ds.batch(idx[i:i + BATCH])
            ts.step(lr, hr)
            total += float(ts.loss)
        return total

    def c_fit_loop(preview_every=10 ** 9):
        meter.reset()
        n = T.run_epoch(model, ts, ds, meter, names, epoch=1, epochs=1, batch_size=BATCH, generator=gen, preview_every=preview_every,
                        preview_dir=folder, log_every=10 ** 9)
        assert n == args.steps

    ms = alternate({"a": a_bare, "b": b_float_every_step, "c": c_fit_loop, "c_aa": c_fit_loop, "d": lambda: c_fit_loop(1)},
                   args.steps, args.repeats)
    rec = meter.read()
    assert rec["loss"]["count"] == args.steps and rec["loss"]["nonfinite"] == 0.0, rec["loss"]
    med = {k: statistics.median(v) for k, v in ms.items()}

    lr, hr = ds.batch(list(range(BATCH)))
    with torch.no_grad():
        sr = model(lr[:1].contiguous())
    values = T.meter_values(ts, names)
    kernels = {k: [] for k in ("meter_update", "preview_strip")}
    for r in range(args.repeats):
        kernels["meter_update"].append(event_us(lambda: meter.update(values, 0), args.kernel_reps))
        kernels["preview_strip"].append(event_us(lambda: T.preview_strip(lr[0], sr[0], hr[0], 1.0), args.kernel_reps))
    for f in os.listdir(folder):
        os.remove(os.path.join(folder, f))
    os.rmdir(folder)
    out = {"workload": f"x{SCALE} LR {LR_SIDE}x{LR_SIDE} batch {BATCH} bf16", "steps": args.steps, "repeats": args.repeats,
           "n_blocks": args.n_blocks, "ms_per_step": summarise(ms), "aa_spread": round(abs(med["c"] - med["c_aa"]) / med["c"], 4),
           "c_minus_a": round((med["c"] - med["a"]) / med["a"], 4), "kernels_us": summarise(kernels)}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
