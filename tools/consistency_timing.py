"""What the LR-consistency term costs the training step, at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16, bf16):
``TrainStep()`` (the plain L1 step, seed fused into the tail backward) against ``TrainStep(lambda_consistency=...)`` (materialised
seed: immediate L1, then m2t_consistency_loss adds into it) and, for comparison on the same build and box, against
``TrainStep(lambda_ssim=...)``, on one model in one process.  The arms alternate, all are warmed up first, every repeat is timed with
device events around `--steps` steps.  Timed stand-alone, by events around `--kernel-reps` back-to-back calls: the term's kernels on a
plan that holds a forward and a seed (forward + fold + backward), its value-only path (forward + fold), and one back-projection
iteration on a contiguous SR batch of the same size against a torch ``copy_`` of the bytes it writes.

Prints one JSON line: ms per step of the arms with their repeats, the repeat-to-repeat spread of the plain arm (the A/A margin of every
comparison made here), the ratios, the stand-alone times, and what the traffic implies at 6.3 TB/s.  Needs a device: without one it
fails.

    python tools/consistency_timing.py [--repeats 5] [--steps 20] [--warmup 3] [--dtype bf16]
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

RESULT_KEYS = ("workload", "dtype", "batch", "repeats", "steps", "lambda_consistency", "lambda_ssim", "ms_per_step", "ms_repeats",
               "l1_spread", "ratio_to_l1", "added_ms", "kernels_ms", "kernels_ms_repeats", "traffic_mb", "implied_ms_at_6_3_tb_s")
ARMS = ("l1", "l1+consistency", "l1+ssim")
KERNELS = ("term", "term_value_only", "back_project_iteration", "copy_of_sr")
STREAM_TB_S = 6.3


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed rounds of (l1, l1 + consistency, l1 + ssim) repeats (at least 3)")
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of every arm before the first repeat")
    ap.add_argument("--kernel-reps", type=int, default=20, help="back-to-back calls per stand-alone timing")
    ap.add_argument("--lambda-consistency", type=float, default=0.1)
    ap.add_argument("--lambda-ssim", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    if args.repeats < 3:
        ap.error("--repeats must be at least 3 (the l1 arm's spread is the margin of the comparison)")
    if min(args.steps, args.batch, args.blocks, args.lr_size, args.kernel_reps) < 1 or args.warmup < 0 \
            or not args.lambda_consistency > 0 or not args.lambda_ssim > 0:
        ap.error("counts, --lambda-consistency and --lambda-ssim must be positive")
    if args.lr_size * 4 < 11:
        ap.error("--lr-size: the SR side must be at least 11 (the SSIM window of the comparison arm)")
    return args


def traffic_mb(batch: int, lr_size: int, scale: int = 4) -> dict:
    """The bytes each piece has to move, in MB: SR planes are fp32, the rho' / residual plane is fp64."""
    sr = batch * 3 * (lr_size * scale) ** 2 * 4 / 1e6
    lr = batch * 3 * lr_size ** 2 * 4 / 1e6
    plane = 2 * lr
    return {"forward": round(sr + lr + plane, 2),                    # x and y read, the plane written
            "backward": round(plane + 3 * sr, 2),                    # the plane and x (the mask) read, the seed read and written
            "back_project_iteration": round(sr + lr + plane + plane + 2 * sr, 2),
            "copy_of_sr": round(2 * sr, 2)}


def result(args, ms: dict, kernel_ms: dict):
    """The JSON line from the per-repeat times: ms = {arm: [ms per step]}, kernel_ms = {name of KERNELS: [ms]}."""
    med = {k: statistics.median(ms[k]) for k in ARMS}
    kmed = {k: statistics.median(kernel_ms[k]) for k in KERNELS}
    mb = traffic_mb(args.batch, args.lr_size)
    implied = {"term": (mb["forward"] + mb["backward"]) / (STREAM_TB_S * 1e3), "term_value_only": mb["forward"] / (STREAM_TB_S * 1e3),
               "back_project_iteration": mb["back_project_iteration"] / (STREAM_TB_S * 1e3), "copy_of_sr": mb["copy_of_sr"] / (STREAM_TB_S * 1e3)}
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, batch {args.batch}: L1 vs L1 + "
                       "lambda_consistency vs L1 + lambda_ssim (1 - SSIM); the term's kernels and one back-projection iteration alone",
           "dtype": args.dtype, "batch": args.batch, "repeats": args.repeats, "steps": args.steps,
           "lambda_consistency": args.lambda_consistency, "lambda_ssim": args.lambda_ssim,
           "ms_per_step": {k: round(med[k], 4) for k in ARMS},
           "ms_repeats": {k: [round(v, 4) for v in ms[k]] for k in ARMS},
           "l1_spread": round((max(ms["l1"]) - min(ms["l1"])) / med["l1"], 4),
           "ratio_to_l1": {k: round(med[k] / med["l1"], 4) for k in ARMS[1:]},
           "added_ms": {k: round(med[k] - med["l1"], 4) for k in ARMS[1:]},
           "kernels_ms": {k: round(kmed[k], 4) for k in KERNELS},
           "kernels_ms_repeats": {k: [round(v, 4) for v in kernel_ms[k]] for k in KERNELS},
           "traffic_mb": mb, "implied_ms_at_6_3_tb_s": {k: round(v, 4) for k, v in implied.items()}}
    assert tuple(out) == RESULT_KEYS
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("consistency_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    # one model: the arms differ in the loss requests alone (the plan, its workspace and the streams are shared)
    model = create_model(margs).to(device)
    arms = {"l1": TrainStep(model, lr=1e-4, world_size=1),
            "l1+consistency": TrainStep(model, lr=1e-4, world_size=1, lambda_consistency=args.lambda_consistency),
            "l1+ssim": TrainStep(model, lr=1e-4, world_size=1, lambda_ssim=args.lambda_ssim)}
    g = torch.Generator(device=device).manual_seed(33)
    Hs, B, n = args.lr_size * 4, args.batch, args.lr_size
    lr = torch.nn.functional.avg_pool2d(torch.rand((B, 3, Hs, Hs), generator=g, device=device), 4).contiguous()
    lib = _lib.load()
    plan = model._plan_for(lr)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    Hp, Wp = plan.query("padded_h") * 4, plan.query("padded_w") * 4
    pre_full = plan.ws_tensor("srpre", dtype=torch.float32).view(B, 3, Hp, Wp)
    pre = pre_full[..., :Hs, :Hs]
    hr = (pre.clamp(0.0, 1.0) + 0.05 * torch.randn(pre.shape, generator=g, device=device)).clamp(0.0, 1.0).contiguous()

    def timed(fn, reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    for ts in arms.values():
        timed(lambda: ts.step(lr, hr), max(1, args.warmup))
    ms = {k: [] for k in ARMS}
    for _ in range(args.repeats):
        for k in ARMS:
            ms[k].append(timed(lambda: arms[k].step(lr, hr), args.steps))

    # the kernels alone: a forward and a materialised seed stay valid across the loss calls
    out = torch.zeros(1, device=device)
    scratch = torch.empty(int(lib.m2t_consistency_scratch_bytes(B, 3, n, n, 4)), dtype=torch.uint8, device=device)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st), "m2t_l1_loss")
    sr = pre.clamp(0.0, 1.0).contiguous()
    other = torch.empty_like(sr)

    def term():
        _lib.check(lib.m2t_consistency_loss(plan.handle, _lib.ptr(lr), args.lambda_consistency, float(lr.numel()), 1.0, 0.0, _lib.ptr(out), 0,
                                            _lib.ptr(scratch), ws, st), "m2t_consistency_loss")

    def value_only():
        _lib.check(lib.m2t_consistency_loss_tensor(_lib.ptr(pre_full), _lib.ptr(lr), B, 3, n, n, 4, 3 * Hp * Wp, Wp, 1.0, 1, 0.0,
                                                   1.0 / lr.numel(), None, _lib.ptr(out), None, 0, _lib.ptr(scratch), st),
                   "m2t_consistency_loss_tensor")

    def back_project():
        _lib.check(lib.m2t_back_project_f32(_lib.ptr(sr), _lib.ptr(lr), B, 3, n, n, 4, 1.0, 1.0, 1, None, _lib.ptr(scratch), st),
                   "m2t_back_project_f32")

    kernel_ms = {}
    for name, call in zip(KERNELS, (term, value_only, back_project, lambda: other.copy_(sr))):
        timed(call, 3)
        kernel_ms[name] = [timed(call, args.kernel_reps) for _ in range(args.repeats)]
    print(json.dumps(result(args, ms, kernel_ms)))


if __name__ == "__main__":
    main()
