"""What the optimizer options cost the training step, at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16):
a plain ``TrainStep`` (one m2t_adam_step) against ``TrainStep(max_grad_norm, weight_decay + decoupled_weight_decay, ema_decay,
skip_nonfinite)`` (m2t_grad_norm's two launches + one m2t_adam_step_ex) in the same process.  The two arms alternate, both are
warmed up first, every repeat is timed with device events around `--steps` steps.  Prints one JSON line: ms per step of either
arm, the repeat-to-repeat spread of the plain arm, the overhead in ms and as a share of the plain step, whether it is within the
plain arm's spread or within 1 % of the step, and the bytes the extra passes move.  Needs a device: without one it fails.

    python tools/optim_timing.py [--repeats 5] [--steps 20] [--warmup 3] [--dtype bf16]
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

RESULT_KEYS = ("workload", "dtype", "batch", "options", "repeats", "steps", "n_params", "plain_ms_per_step", "optim_ms_per_step",
               "plain_ms_repeats", "optim_ms_repeats", "plain_spread", "overhead_ms", "overhead_share", "extra_bytes",
               "arrays_plain", "arrays_optim", "overhead_within_plain_spread", "overhead_within_1_percent")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed pairs of (plain, with options) repeats (at least 5)")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of either arm before the first repeat")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--weight-decay", type=float, default=1e-2)
    ap.add_argument("--ema-decay", type=float, default=0.999)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5 (the plain arm's spread is the margin of the comparison)")
    if min(args.steps, args.batch, args.blocks, args.lr_size) < 1 or args.warmup < 0:
        ap.error("counts must be positive")
    return args


def options(args) -> dict:
    """The keyword arguments of the arm with options: clip + decoupled decay + EMA + skip."""
    return {"max_grad_norm": args.max_grad_norm, "weight_decay": args.weight_decay, "decoupled_weight_decay": True,
            "ema_decay": args.ema_decay, "skip_nonfinite": True}


def shapes(args, scale: int = 4):
    return (args.batch, 3, args.lr_size, args.lr_size), (args.batch, 3, args.lr_size * scale, args.lr_size * scale)


def traffic(n_params: int, ema: bool = True, norm: bool = True):
    """(arrays of 4 n bytes the plain Adam pass moves, arrays with the options, extra bytes): Adam reads p, g, m, v and writes
    p, m, v (7); the norm reads g once more (+1), the EMA is read and written (+2)."""
    plain = 7
    optim = plain + (1 if norm else 0) + (2 if ema else 0)
    return plain, optim, (optim - plain) * 4 * int(n_params)


def result(args, plain_ms, optim_ms, n_params: int):
    """The JSON line from the per-repeat times (ms per step of either arm)."""
    p, o = statistics.median(plain_ms), statistics.median(optim_ms)
    spread = (max(plain_ms) - min(plain_ms)) / p
    a_plain, a_optim, extra = traffic(n_params)
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, batch {args.batch}: plain "
                       "TrainStep vs clip + decoupled decay + EMA + skip_nonfinite",
           "dtype": args.dtype, "batch": args.batch, "options": options(args), "repeats": args.repeats, "steps": args.steps,
           "n_params": int(n_params), "plain_ms_per_step": round(p, 4), "optim_ms_per_step": round(o, 4),
           "plain_ms_repeats": [round(v, 4) for v in plain_ms], "optim_ms_repeats": [round(v, 4) for v in optim_ms],
           "plain_spread": round(spread, 4), "overhead_ms": round(o - p, 4), "overhead_share": round((o - p) / p, 4),
           "extra_bytes": extra, "arrays_plain": a_plain, "arrays_optim": a_optim,
           "overhead_within_plain_spread": bool(o <= p * (1.0 + spread)), "overhead_within_1_percent": bool(o <= p * 1.01)}
    assert tuple(out) == RESULT_KEYS
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    ts_plain = TrainStep(create_model(margs).to(device), lr=1e-4, world_size=1)
    ts_optim = TrainStep(create_model(margs).to(device), lr=1e-4, world_size=1, **options(args))
    lr_shape, hr_shape = shapes(args)
    g = torch.Generator(device=device).manual_seed(33)
    hr = torch.rand(hr_shape, generator=g, device=device)
    lr = torch.nn.functional.avg_pool2d(hr, 4).contiguous()
    assert tuple(lr.shape) == lr_shape

    def timed(ts, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            ts.step(lr, hr)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    for ts in (ts_plain, ts_optim):
        timed(ts, max(1, args.warmup))
    plain_ms, optim_ms = [], []
    for _ in range(args.repeats):
        plain_ms.append(timed(ts_plain, args.steps))
        optim_ms.append(timed(ts_optim, args.steps))
    out = result(args, plain_ms, optim_ms, ts_plain.grads.numel())
    out["skipped_steps"] = int(ts_optim.skipped_steps.item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
