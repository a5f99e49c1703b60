"""What the frequency-domain loss term costs the training step, at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16,
bf16): ``TrainStep()`` (the plain L1 step, seed fused into the tail backward) against ``TrainStep(lambda_fft=0.1)`` (materialised
seed: immediate L1, then m2t_fft_loss adds into it) on one model in one process.  The two arms alternate, both are warmed up first,
every repeat is timed with device events around `--steps` steps.  The launches of m2t_fft_loss (rows forward, columns forward +
signs + adjoint, rows adjoint, the fold of the partial sums) are also timed stand-alone, by events around `--kernel-reps`
back-to-back calls on a plan that holds a forward and a seed, and each of the three kernels by name through torch.profiler's
device activity records over the same calls (`--no-kernel-profile` leaves that out; if the profiler gives no device records the
line says so in "kernel_ms_error").  Prints one JSON line.  Needs a device: without one it fails.

    python tools/fft_loss_timing.py [--repeats 5] [--steps 20] [--warmup 3] [--dtype bf16] [--norm backward]
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

RESULT_KEYS = ("workload", "dtype", "batch", "repeats", "steps", "lambda_fft", "fft_norm", "ms_per_step", "ms_repeats", "l1_spread",
               "ratio_to_l1", "added_ms", "fft_kernels_ms", "fft_kernels_ms_repeats", "kernel_ms", "kernel_ms_error")
KERNELS = ("fft_rows_fwd_kernel", "fft_cols_kernel", "fft_rows_adj_kernel", "fft_loss_finish_kernel")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed pairs of (l1, l1 + fft) repeats (at least 3)")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of every arm before the first repeat")
    ap.add_argument("--kernel-reps", type=int, default=20, help="back-to-back m2t_fft_loss calls per stand-alone timing")
    ap.add_argument("--lambda-fft", type=float, default=0.1)
    ap.add_argument("--norm", default="backward", choices=["backward", "ortho"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-kernel-profile", action="store_true", help="skip the per-kernel times (torch.profiler)")
    args = ap.parse_args(argv)
    if args.repeats < 3:
        ap.error("--repeats must be at least 3 (the l1 arm's spread is the margin of the comparison)")
    if min(args.steps, args.batch, args.blocks, args.lr_size, args.kernel_reps) < 1 or args.warmup < 0 or not args.lambda_fft > 0:
        ap.error("counts and --lambda-fft must be positive")
    return args


def result(args, l1_ms: list, fft_ms: list, kernel_ms: list, per_kernel, per_kernel_error):
    """The JSON line from the per-repeat times."""
    l1, ff = statistics.median(l1_ms), statistics.median(fft_ms)
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, batch {args.batch}: L1 vs L1 + "
                       "lambda_fft mean |rfft2(sr - hr)|",
           "dtype": args.dtype, "batch": args.batch, "repeats": args.repeats, "steps": args.steps, "lambda_fft": args.lambda_fft,
           "fft_norm": args.norm,
           "ms_per_step": {"l1": round(l1, 4), "l1+fft": round(ff, 4)},
           "ms_repeats": {"l1": [round(v, 4) for v in l1_ms], "l1+fft": [round(v, 4) for v in fft_ms]},
           "l1_spread": round((max(l1_ms) - min(l1_ms)) / l1, 4), "ratio_to_l1": round(ff / l1, 4), "added_ms": round(ff - l1, 4),
           "fft_kernels_ms": round(statistics.median(kernel_ms), 4), "fft_kernels_ms_repeats": [round(v, 4) for v in kernel_ms],
           "kernel_ms": per_kernel, "kernel_ms_error": per_kernel_error}
    assert tuple(out) == RESULT_KEYS
    return out


def per_kernel_times(fn, reps):
    """{kernel: mean ms per launch} of the library's FFT kernels over `reps` calls of fn, from torch.profiler's device records."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for k in KERNELS:
            if k in ev.key:
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total")
                out[k] = round(out.get(k, 0.0) + float(total) / 1000.0 / reps, 4)
    if not out:
        raise RuntimeError("torch.profiler returned no device record of the FFT kernels")
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fft_loss_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    # one model: the arms differ in the loss requests alone (the plan, its workspace and the streams are shared)
    model = create_model(margs).to(device)
    arms = {"l1": TrainStep(model, lr=1e-4, world_size=1),
            "l1+fft": TrainStep(model, lr=1e-4, world_size=1, lambda_fft=args.lambda_fft, fft_norm=args.norm)}
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
    l1_ms, fft_ms = [], []
    for _ in range(args.repeats):
        l1_ms.append(timed(lambda: arms["l1"].step(lr, hr), args.steps))
        fft_ms.append(timed(lambda: arms["l1+fft"].step(lr, hr), args.steps))

    # the kernels alone: a forward and a materialised seed stay valid across m2t_fft_loss calls
    lib = _lib.load()
    plan = model._plan_for(lr)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    out = torch.zeros(1, device=device)
    B, _, Hs, Ws = hr.shape
    scratch = torch.empty(int(lib.m2t_fft_loss_scratch_bytes(B, 3, Hs, Ws)), dtype=torch.uint8, device=device)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st), "m2t_l1_loss")
    divisor = float(2 * B * 3 * Hs * (Ws // 2 + 1))
    norm = _lib.FFT_NORMS[args.norm]

    def fft_call():
        _lib.check(lib.m2t_fft_loss(plan.handle, _lib.ptr(hr), args.lambda_fft, divisor, 1.0, norm, _lib.ptr(out), 0, _lib.ptr(scratch), ws, st),
                   "m2t_fft_loss")

    timed(fft_call, 3)
    kernel_ms = [timed(fft_call, args.kernel_reps) for _ in range(args.repeats)]
    per_kernel, err = None, None
    if args.no_kernel_profile:
        err = "not requested"
    else:
        try:
            per_kernel = per_kernel_times(fft_call, args.kernel_reps)
        except Exception as e:                                      # the profiler is a convenience of this tool, not of the product
            err = f"{type(e).__name__}: {e}"
    print(json.dumps(result(args, l1_ms, fft_ms, kernel_ms, per_kernel, err)))


if __name__ == "__main__":
    main()
