"""What the wavelet-domain loss term costs the training step, at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16, bf16):
``TrainStep()`` (the plain L1 step, seed fused into the tail backward) against ``TrainStep(lambda_wavelet=..., wavelet='db2', wavelet_levels=2)`` (materialised seed:
immediate L1, then m2t_wavelet_loss adds into it; default band weights) and, for comparison on the same build and box, against ``TrainStep(lambda_ssim=...)``,
on one model in one process.  The arms alternate, all are warmed up first, every repeat is timed with device events around `--steps`
steps.  The kernels of both terms are also timed stand-alone, by events around `--kernel-reps` back-to-back m2t_wavelet_loss /
m2t_ssim_loss calls on a plan that holds a forward and a seed.

The target is built from the model's own pre-clamp output (HR = clamp(clamp(pre) + 0.05 randn)), the pair the other timing tools
use; the term's value during the stand-alone timing is part of the result, next to the HBM traffic the kernels' structure implies.

Prints one JSON line: ms per step of the arms with their repeats, the repeat-to-repeat spread of the plain arm (the A/A margin of
every comparison made here), the ratios, and the stand-alone times.  Needs a device: without one it fails.

    python tools/wavelet_loss_timing.py [--repeats 5] [--steps 20] [--warmup 3] [--dtype bf16]
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

RESULT_KEYS = ("workload", "dtype", "batch", "repeats", "steps", "lambda_wavelet", "wavelet", "wavelet_levels", "lambda_ssim", "ms_per_step",
               "ms_repeats", "l1_spread", "ratio_to_l1", "added_ms", "wavelet_kernels_ms", "wavelet_kernels_ms_repeats", "ssim_kernels_ms",
               "ssim_kernels_ms_repeats", "wavelet_to_ssim_kernels", "wavelet_hbm_bytes", "wavelet_value")
ARMS = ("l1", "l1+wavelet", "l1+ssim")
WAVELET, LEVELS = "db2", 2


def hbm_bytes_per_pixel_channel(levels: int) -> int:
    """What the kernels move through HBM per (pixel, channel) with the default weights (every detail band on, LL off); DESIGN.md has
    the derivation: level 1 reads x and y (8) and writes LL and three psi planes (32); each further level reads LL (8) and writes
    three psi planes, and LL unless it is the last (24 or 32); the backward reads three psi planes per level and abar_j below the
    last (24 or 32) and writes abar_{j-1} (8), level 1 instead reading x and read-add-writing the seed (12)."""
    fwd = 8 + 32 if levels > 1 else 8 + 24
    for j in range(2, levels + 1):
        fwd += 8 + (32 if j < levels else 24)
    bwd = 0
    for j in range(levels, 0, -1):
        bwd += (24 if j == levels else 32) + (8 if j > 1 else 12)
    return fwd + bwd


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed rounds of (l1, l1 + wavelet, l1 + ssim) repeats (at least 3)")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of every arm before the first repeat")
    ap.add_argument("--kernel-reps", type=int, default=20, help="back-to-back loss calls per stand-alone timing")
    ap.add_argument("--lambda-wavelet", type=float, default=0.1)
    ap.add_argument("--lambda-ssim", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    if args.repeats < 3:
        ap.error("--repeats must be at least 3 (the l1 arm's spread is the margin of the comparison)")
    if min(args.steps, args.batch, args.blocks, args.lr_size, args.kernel_reps) < 1 or args.warmup < 0 \
            or not args.lambda_wavelet > 0 or not args.lambda_ssim > 0:
        ap.error("counts, --lambda-wavelet and --lambda-ssim must be positive")
    if args.lr_size * 4 < 11:
        ap.error("--lr-size: the SR side must be at least 11 (the SSIM window of the comparison arm)")
    return args


def result(args, ms: dict, kernel_ms: dict, value: float):
    """The JSON line from the per-repeat times: ms = {arm: [ms per step]}, kernel_ms = {"wavelet": [...], "ssim": [...]}."""
    med = {k: statistics.median(ms[k]) for k in ARMS}
    kmed = {k: statistics.median(v) for k, v in kernel_ms.items()}
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, batch {args.batch}: L1 vs L1 + "
                       f"lambda_wavelet ({WAVELET}, {LEVELS} levels) vs L1 + lambda_ssim (1 - SSIM)",
           "dtype": args.dtype, "batch": args.batch, "repeats": args.repeats, "steps": args.steps,
           "lambda_wavelet": args.lambda_wavelet, "wavelet": WAVELET, "wavelet_levels": LEVELS, "lambda_ssim": args.lambda_ssim,
           "ms_per_step": {k: round(med[k], 4) for k in ARMS},
           "ms_repeats": {k: [round(v, 4) for v in ms[k]] for k in ARMS},
           "l1_spread": round((max(ms["l1"]) - min(ms["l1"])) / med["l1"], 4),
           "ratio_to_l1": {k: round(med[k] / med["l1"], 4) for k in ARMS[1:]},
           "added_ms": {k: round(med[k] - med["l1"], 4) for k in ARMS[1:]},
           "wavelet_kernels_ms": round(kmed["wavelet"], 4), "wavelet_kernels_ms_repeats": [round(v, 4) for v in kernel_ms["wavelet"]],
           "ssim_kernels_ms": round(kmed["ssim"], 4), "ssim_kernels_ms_repeats": [round(v, 4) for v in kernel_ms["ssim"]],
           "wavelet_to_ssim_kernels": round(kmed["wavelet"] / kmed["ssim"], 4),
           "wavelet_hbm_bytes": hbm_bytes_per_pixel_channel(LEVELS) * args.batch * 3 * (args.lr_size * 4) ** 2, "wavelet_value": round(value, 6)}
    assert tuple(out) == RESULT_KEYS
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wavelet_loss_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep, resolve_wavelet, wavelet_call_args
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    # one model: the arms differ in the loss requests alone (the plan, its workspace and the streams are shared)
    model = create_model(margs).to(device)
    arms = {"l1": TrainStep(model, lr=1e-4, world_size=1),
            "l1+wavelet": TrainStep(model, lr=1e-4, world_size=1, lambda_wavelet=args.lambda_wavelet, wavelet=WAVELET, wavelet_levels=LEVELS),
            "l1+ssim": TrainStep(model, lr=1e-4, world_size=1, lambda_ssim=args.lambda_ssim)}
    g = torch.Generator(device=device).manual_seed(33)
    Hs = args.lr_size * 4
    lr = torch.nn.functional.avg_pool2d(torch.rand((args.batch, 3, Hs, Hs), generator=g, device=device), 4).contiguous()
    lib = _lib.load()
    plan = model._plan_for(lr)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    Hp, Wp = plan.query("padded_h") * 4, plan.query("padded_w") * 4
    pre = plan.ws_tensor("srpre", dtype=torch.float32).view(args.batch, 3, Hp, Wp)[..., :Hs, :Hs]
    hr = (pre.clamp(0.0, 1.0) + 0.05 * torch.randn(pre.shape, generator=g, device=device)).clamp(0.0, 1.0).contiguous()

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
    ms = {k: [] for k in ARMS}
    for _ in range(args.repeats):
        for k in ARMS:
            ms[k].append(timed(lambda: arms[k].step(lr, hr), args.steps))

    # the kernels alone: a forward and a materialised seed stay valid across the loss calls
    out = torch.zeros(1, device=device)
    B = args.batch
    wargs = wavelet_call_args(resolve_wavelet(WAVELET, LEVELS))
    s_wv = torch.empty(int(lib.m2t_wavelet_loss_scratch_bytes(B, 3, Hs, Hs, LEVELS, wargs[2])), dtype=torch.uint8, device=device)
    s_ss = torch.empty(int(lib.m2t_ssim_loss_scratch_bytes(B, 3, Hs, Hs)), dtype=torch.uint8, device=device)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st), "m2t_l1_loss")

    def wavelet_call():
        _lib.check(lib.m2t_wavelet_loss(plan.handle, _lib.ptr(hr), args.lambda_wavelet, float(hr.numel()), 1.0, *wargs, _lib.ptr(out), 0,
                                        _lib.ptr(s_wv), ws, st), "m2t_wavelet_loss")

    def ssim_call():
        _lib.check(lib.m2t_ssim_loss(plan.handle, _lib.ptr(hr), args.lambda_ssim, float(B * 3 * (Hs - 10) * (Hs - 10)), 1.0, _lib.ptr(out),
                                     0, _lib.ptr(s_ss), ws, st), "m2t_ssim_loss")

    kernel_ms = {}
    for name, call in (("wavelet", wavelet_call), ("ssim", ssim_call)):
        timed(call, 3)
        kernel_ms[name] = [timed(call, args.kernel_reps) for _ in range(args.repeats)]
    timed(wavelet_call, 1)
    print(json.dumps(result(args, ms, kernel_ms, float(out))))


if __name__ == "__main__":
    main()
