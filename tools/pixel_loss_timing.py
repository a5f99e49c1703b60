"""What a pixel loss other than L1 costs the training step, at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16,
bf16): ``TrainStep()`` (l1) against ``TrainStep(pixel_loss=kind)`` for mse, charbonnier and smooth_l1 in the same process.  Every kind
runs the launches of the L1 step (the seed is taken inside the fused tail backward); the difference is a few VALU operations per HR
pixel.  The l1 arm alternates with each other kind, all arms are warmed up first, every repeat is timed with device events around
`--steps` steps.  Prints one JSON line: ms per step of every kind (l1: over all its repeats), the repeat-to-repeat spread of the l1
arm, and each kind's ratio to the l1 repeats it alternated with.  Needs a device: without one it fails.

    python tools/pixel_loss_timing.py [--repeats 5] [--steps 20] [--warmup 3] [--dtype bf16]
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

KINDS = (("mse", None), ("charbonnier", 1e-6), ("smooth_l1", 1.0))
RESULT_KEYS = ("workload", "dtype", "batch", "repeats", "steps", "fused_l1", "ms_per_step", "ms_repeats", "l1_spread", "ratio_to_l1",
               "within_l1_spread")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed pairs of (l1, kind) repeats per kind (at least 3)")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of every arm before the first repeat")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    if args.repeats < 3:
        ap.error("--repeats must be at least 3 (the l1 arm's spread is the margin of the comparison)")
    if min(args.steps, args.batch, args.blocks, args.lr_size) < 1 or args.warmup < 0:
        ap.error("counts must be positive")
    return args


def result(args, l1_ms: dict, kind_ms: dict, fused: int):
    """The JSON line from the per-repeat times: l1_ms[kind] are the l1 repeats that alternated with kind_ms[kind]."""
    all_l1 = [v for k in kind_ms for v in l1_ms[k]]
    l1 = statistics.median(all_l1)
    spread = (max(all_l1) - min(all_l1)) / l1
    ms = {"l1": round(l1, 4)}
    reps = {"l1": [round(v, 4) for v in all_l1]}
    ratio, within = {}, {}
    for k, vals in kind_ms.items():
        m = statistics.median(vals)
        ms[k] = round(m, 4)
        reps[k] = [round(v, 4) for v in vals]
        ratio[k] = round(m / statistics.median(l1_ms[k]), 4)
        within[k] = bool(m <= statistics.median(l1_ms[k]) * (1.0 + spread))
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, batch {args.batch}: pixel loss l1 "
                       "vs mse / charbonnier / smooth_l1",
           "dtype": args.dtype, "batch": args.batch, "repeats": args.repeats, "steps": args.steps, "fused_l1": int(fused),
           "ms_per_step": ms, "ms_repeats": reps, "l1_spread": round(spread, 4), "ratio_to_l1": ratio, "within_l1_spread": within}
    assert tuple(out) == RESULT_KEYS
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pixel_loss_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    # one model: the arms differ in the loss request alone (the plan, its workspace and the streams are shared)
    model = create_model(margs).to(device)
    arms = {"l1": TrainStep(model, lr=1e-4, world_size=1)}
    for kind, param in KINDS:
        arms[kind] = TrainStep(model, lr=1e-4, world_size=1, pixel_loss=kind, pixel_loss_param=param)
    g = torch.Generator(device=device).manual_seed(33)
    hr = torch.rand((args.batch, 3, args.lr_size * 4, args.lr_size * 4), generator=g, device=device)
    lr = torch.nn.functional.avg_pool2d(hr, 4).contiguous()

    def timed(ts, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            ts.step(lr, hr)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    for ts in arms.values():
        timed(ts, max(1, args.warmup))
    l1_ms = {k: [] for k, _ in KINDS}
    kind_ms = {k: [] for k, _ in KINDS}
    for _ in range(args.repeats):
        for kind, _p in KINDS:
            l1_ms[kind].append(timed(arms["l1"], args.steps))
            kind_ms[kind].append(timed(arms[kind], args.steps))
    fused = model._plan_for(lr).query("opt:fused_l1")
    print(json.dumps(result(args, l1_ms, kind_ms, fused)))


if __name__ == "__main__":
    main()
