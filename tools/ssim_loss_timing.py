"""What the structural loss term costs the training step, at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16,
bf16): ``TrainStep()`` (the plain L1 step, seed fused into the tail backward) against ``TrainStep(lambda_ssim=0.1)`` (materialised
seed: immediate L1, then m2t_ssim_loss adds into it) on one model in one process.  The two arms alternate, both are warmed up first,
every repeat is timed with device events around `--steps` steps.  The SSIM kernels (tile kernel + the fold of the partial sums) are
also timed stand-alone, by events around `--kernel-reps` back-to-back m2t_ssim_loss calls on a plan that holds a forward and a seed.
Prints one JSON line: ms per step of both arms with their repeats, the repeat-to-repeat spread of the plain arm, the ratio, and the
stand-alone time.  Needs a device: without one it fails.

    python tools/ssim_loss_timing.py [--repeats 5] [--steps 20] [--warmup 3] [--dtype bf16]
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

RESULT_KEYS = ("workload", "dtype", "batch", "repeats", "steps", "lambda_ssim", "ms_per_step", "ms_repeats", "l1_spread", "ratio_to_l1",
               "added_ms", "ssim_kernels_ms", "ssim_kernels_ms_repeats")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed pairs of (l1, l1 + ssim) repeats (at least 3)")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of every arm before the first repeat")
    ap.add_argument("--kernel-reps", type=int, default=20, help="back-to-back m2t_ssim_loss calls per stand-alone timing")
    ap.add_argument("--lambda-ssim", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    if args.repeats < 3:
        ap.error("--repeats must be at least 3 (the l1 arm's spread is the margin of the comparison)")
    if min(args.steps, args.batch, args.blocks, args.lr_size, args.kernel_reps) < 1 or args.warmup < 0 or not args.lambda_ssim > 0:
        ap.error("counts and --lambda-ssim must be positive")
    return args


def result(args, l1_ms: list, ssim_ms: list, kernel_ms: list):
    """The JSON line from the per-repeat times."""
    l1, ss = statistics.median(l1_ms), statistics.median(ssim_ms)
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, batch {args.batch}: L1 vs L1 + "
                       "lambda_ssim (1 - SSIM)",
           "dtype": args.dtype, "batch": args.batch, "repeats": args.repeats, "steps": args.steps, "lambda_ssim": args.lambda_ssim,
           "ms_per_step": {"l1": round(l1, 4), "l1+ssim": round(ss, 4)},
           "ms_repeats": {"l1": [round(v, 4) for v in l1_ms], "l1+ssim": [round(v, 4) for v in ssim_ms]},
           "l1_spread": round((max(l1_ms) - min(l1_ms)) / l1, 4), "ratio_to_l1": round(ss / l1, 4), "added_ms": round(ss - l1, 4),
           "ssim_kernels_ms": round(statistics.median(kernel_ms), 4), "ssim_kernels_ms_repeats": [round(v, 4) for v in kernel_ms]}
    assert tuple(out) == RESULT_KEYS
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ssim_loss_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    # one model: the arms differ in the loss requests alone (the plan, its workspace and the streams are shared)
    model = create_model(margs).to(device)
    arms = {"l1": TrainStep(model, lr=1e-4, world_size=1), "l1+ssim": TrainStep(model, lr=1e-4, world_size=1, lambda_ssim=args.lambda_ssim)}
    g = torch.Generator(device=device).manual_seed(33)
    hr = torch.rand((args.batch, 3, args.lr_size * 4, args.lr_size * 4), generator=g, device=device)
    lr = torch.nn.functional.avg_pool2d(hr, 4).contiguous()

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    for ts in arms.values():
        timed(lambda: ts.step(lr, hr), max(1, args.warmup))
    l1_ms, ssim_ms = [], []
    for _ in range(args.repeats):
        l1_ms.append(timed(lambda: arms["l1"].step(lr, hr), args.steps))
        ssim_ms.append(timed(lambda: arms["l1+ssim"].step(lr, hr), args.steps))

    # the kernels alone: a forward and a materialised seed stay valid across m2t_ssim_loss calls
    lib = _lib.load()
    plan = model._plan_for(lr)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    out = torch.zeros(1, device=device)
    B, _, Hs, Ws = hr.shape
    scratch = torch.empty(int(lib.m2t_ssim_loss_scratch_bytes(B, 3, Hs, Ws)), dtype=torch.uint8, device=device)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st), "m2t_l1_loss")
    divisor = float(B * 3 * (Hs - 10) * (Ws - 10))

    def ssim_call():
        _lib.check(lib.m2t_ssim_loss(plan.handle, _lib.ptr(hr), args.lambda_ssim, divisor, 1.0, _lib.ptr(out), 0, _lib.ptr(scratch), ws, st),
                   "m2t_ssim_loss")

    timed(ssim_call, 3)
    kernel_ms = [timed(ssim_call, args.kernel_reps) for _ in range(args.repeats)]
    print(json.dumps(result(args, l1_ms, ssim_ms, kernel_ms)))


if __name__ == "__main__":
    main()
