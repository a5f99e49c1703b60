"""BASELINE.json configs[3]'s whole workload on ONE device: x4, 8 blocks, 128^2 LR, global batch 256 as
TrainStep(accum_steps=8) x 32 (8 forward + backward, 7 accumulate passes, 1 Adam), against eight consecutive plain batch-32
``step`` calls (8 forward + backward, 8 Adam: the path as it is without accumulation) in the same process.  The two arms
alternate, both are warmed up first (the plan shape is the same: batch 32), every repeat is timed with device events around
`--cycles` optimizer steps of the accumulated arm / `--cycles` x 8 plain steps.  Prints one JSON line: ms per optimizer step
(accumulated) and per eight plain steps, HR patches / s at effective batch 256, the repeat-to-repeat spread of the plain arm and
whether the accumulated arm is within it.  Needs a device: without one it fails.

    python tools/accum_timing.py [--repeats 5] [--cycles 10] [--warmup 2] [--dtype bf16]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESULT_KEYS = ("workload", "dtype", "accum_steps", "micro_batch", "effective_batch", "repeats", "cycles",
               "accum_ms_per_optimizer_step", "plain_ms_per_k_plain_steps", "accum_ms_repeats", "plain_ms_repeats",
               "accum_patches_per_s", "plain_patches_per_s", "plain_spread", "accum_over_plain", "accum_within_plain_spread")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats per arm (at least 5)")
    ap.add_argument("--cycles", type=int, default=10, help="optimizer steps of the accumulated arm per timed repeat")
    ap.add_argument("--warmup", type=int, default=2, help="untimed optimizer steps (accumulated) / x8 plain steps before the first repeat")
    ap.add_argument("--accum-steps", type=int, default=8)
    ap.add_argument("--micro-batch", type=int, default=32)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5 (the plain arm's spread is the margin of the comparison)")
    if min(args.cycles, args.accum_steps, args.micro_batch, args.blocks) < 1 or args.warmup < 0:
        ap.error("counts must be positive")
    return args


def shapes(args, scale: int = 4):
    """(LR shape, HR shape) of the effective batch; each micro-batch / plain step takes `micro_batch` consecutive samples."""
    B = args.accum_steps * args.micro_batch
    return (B, 3, args.lr_size, args.lr_size), (B, 3, args.lr_size * scale, args.lr_size * scale)


def result(args, accum_ms, plain_ms):
    """The JSON line from the per-repeat times (ms per optimizer step of the accumulated arm, ms per accum_steps plain steps)."""
    B = args.accum_steps * args.micro_batch
    a, p = statistics.median(accum_ms), statistics.median(plain_ms)
    spread = (max(plain_ms) - min(plain_ms)) / p
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, effective batch {B} on one device: "
                       f"accum_steps={args.accum_steps} x {args.micro_batch} vs {args.accum_steps} plain batch-{args.micro_batch} steps",
           "dtype": args.dtype, "accum_steps": args.accum_steps, "micro_batch": args.micro_batch, "effective_batch": B,
           "repeats": args.repeats, "cycles": args.cycles,
           "accum_ms_per_optimizer_step": round(a, 3), "plain_ms_per_k_plain_steps": round(p, 3),
           "accum_ms_repeats": [round(v, 3) for v in accum_ms], "plain_ms_repeats": [round(v, 3) for v in plain_ms],
           "accum_patches_per_s": round(B / a * 1e3, 1), "plain_patches_per_s": round(B / p * 1e3, 1),
           "plain_spread": round(spread, 4), "accum_over_plain": round(a / p, 4),
           "accum_within_plain_spread": bool(a <= p * (1.0 + spread))}
    assert tuple(out) == RESULT_KEYS
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("accum_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    k, b = args.accum_steps, args.micro_batch
    ts_acc = TrainStep(create_model(margs).to(device), lr=1e-4, world_size=1, accum_steps=k)
    ts_plain = TrainStep(create_model(margs).to(device), lr=1e-4, world_size=1)
    lr_shape, hr_shape = shapes(args)
    g = torch.Generator(device=device).manual_seed(33)
    hr = torch.rand(hr_shape, generator=g, device=device)
    lr = torch.nn.functional.avg_pool2d(hr, 4).contiguous()
    assert tuple(lr.shape) == lr_shape

    def accum_arm(n):
        for _ in range(n):
            ts_acc.step(lr, hr)

    def plain_arm(n):
        for _ in range(n):
            for i in range(k):
                ts_plain.step(lr[i * b:(i + 1) * b], hr[i * b:(i + 1) * b])

    def timed(arm):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        arm(args.cycles)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / args.cycles

    accum_arm(max(1, args.warmup))
    plain_arm(max(1, args.warmup))
    torch.cuda.synchronize()
    accum_ms, plain_ms = [], []
    for _ in range(args.repeats):
        accum_ms.append(timed(accum_arm))
        plain_ms.append(timed(plain_arm))
    print(json.dumps(result(args, accum_ms, plain_ms)))


if __name__ == "__main__":
    main()
