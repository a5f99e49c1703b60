"""What the VGG19 feature loss term costs the training step, at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16,
bf16; SR 512 x 512): ``TrainStep()`` (the plain L1 step, seed fused into the tail backward) against
``TrainStep(perceptual_loss=..., lambda_perceptual=...)`` (materialised seed: immediate L1, then m2t_vgg_loss adds into it), on one model
in one process.  The arms alternate (the L1 arm twice per round: its two readings are the A/A spread of the box), all are warmed up
first, every repeat is timed with device events around `--steps` steps.  Also timed, with events around back-to-back calls:

* the term's kernels alone (m2t_vgg_loss on a plan that holds a forward and a seed), full size;
* ``PerceptualLoss(resize=True)`` forward + backward through the module on the same SR / HR pair (224 x 224 inside; the training
  step itself takes resize=False only);
* every MFMA convolution layer (m2t_vgg_conv_forward, m2t_vgg_conv_backward) at the size it has in the full-size term, with the achieved
  TFLOP/s (2 * 9 * Cin * Cout * H * W * N per call) beside the ~2500 TFLOP/s dense bf16 MFMA peak of the MI355X.

The weights are random (He): timing does not depend on them.  Prints one JSON line.  Needs a device: without one it fails.

    python tools/perceptual_timing.py [--repeats 5] [--steps 10] [--warmup 2]
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

PEAK_BF16_TFLOPS = 2500.0
RESULT_KEYS = ("workload", "batch", "repeats", "steps", "lambda_perceptual", "ms_per_step", "ms_repeats", "l1_aa_spread", "ratio_to_l1",
               "added_ms", "term_kernels_ms", "term_kernels_ms_repeats", "term_tflops", "resize_module_ms", "layers", "peak_bf16_tflops")
ARMS = ("l1", "l1+perceptual", "l1_again")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed rounds of (l1, l1 + perceptual, l1) repeats (at least 3)")
    ap.add_argument("--steps", type=int, default=10, help="training steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps of every arm before the first repeat")
    ap.add_argument("--kernel-reps", type=int, default=5, help="back-to-back calls per stand-alone timing")
    ap.add_argument("--lambda-perceptual", type=float, default=0.05)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    args = ap.parse_args(argv)
    if args.repeats < 3:
        ap.error("--repeats must be at least 3 (the l1 arm's spread is the margin of the comparison)")
    if min(args.steps, args.batch, args.blocks, args.lr_size, args.kernel_reps) < 1 or args.warmup < 0 or not args.lambda_perceptual > 0:
        ap.error("counts and --lambda-perceptual must be positive")
    if args.lr_size * 4 < 16:
        ap.error("--lr-size: the SR side must be at least 16")
    return args


def term_flops(batch: int, side: int) -> float:
    """FLOP of one full-size term: the forward of 2 * batch images and the data gradient of batch images (conv1_1 included)."""
    from m2trans_amd import _lib
    cin = (3,) + _lib.VGG_CHANNELS[:-1]
    per_image = sum(2.0 * 9 * ci * co * (side >> lv) ** 2 for ci, co, lv in zip(cin, _lib.VGG_CHANNELS, _lib.VGG_LEVEL))
    return 3.0 * batch * per_image


def result(args, ms: dict, term_ms: list, resize_ms: list, layers: list):
    med = {k: statistics.median(ms[k]) for k in ARMS}
    l1 = 0.5 * (med["l1"] + med["l1_again"])
    tmed = statistics.median(term_ms)
    out = {"workload": f"x4 SR train step, {args.lr_size}x{args.lr_size} LR, {args.blocks} blocks, batch {args.batch}, bf16: L1 vs L1 + "
                       "lambda_perceptual (VGG19 features, L1 criterion, five taps)",
           "batch": args.batch, "repeats": args.repeats, "steps": args.steps, "lambda_perceptual": args.lambda_perceptual,
           "ms_per_step": {k: round(med[k], 4) for k in ARMS},
           "ms_repeats": {k: [round(v, 4) for v in ms[k]] for k in ARMS},
           "l1_aa_spread": round(abs(med["l1"] - med["l1_again"]) / l1, 4),
           "ratio_to_l1": round(med["l1+perceptual"] / l1, 4), "added_ms": round(med["l1+perceptual"] - l1, 4),
           "term_kernels_ms": round(tmed, 4), "term_kernels_ms_repeats": [round(v, 4) for v in term_ms],
           "term_tflops": round(term_flops(args.batch, args.lr_size * 4) / (tmed * 1e-3) / 1e12, 2),
           "resize_module_ms": round(statistics.median(resize_ms), 4), "layers": layers, "peak_bf16_tflops": PEAK_BF16_TFLOPS}
    assert tuple(out) == RESULT_KEYS
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.losses import PerceptualLoss, vgg_param_names
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    cin = (3,) + _lib.VGG_CHANNELS[:-1]
    sd = {}
    for name, ci, co in zip(vgg_param_names()[::2], cin, _lib.VGG_CHANNELS):
        sd[name] = torch.randn(co, ci, 3, 3) * (2.0 / (9 * ci)) ** 0.5
        sd[name.replace("weight", "bias")] = torch.randn(co) * 0.05
    tower = PerceptualLoss(device=device).load_vgg_state_dict(sd)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype="bf16")
    model = create_model(margs).to(device)
    arms = {"l1": TrainStep(model, lr=1e-4, world_size=1),
            "l1+perceptual": TrainStep(model, lr=1e-4, world_size=1, perceptual_loss=tower, lambda_perceptual=args.lambda_perceptual)}
    arms["l1_again"] = arms["l1"]
    g = torch.Generator(device=device).manual_seed(33)
    B, Hs = args.batch, args.lr_size * 4
    lr = torch.nn.functional.avg_pool2d(torch.rand((B, 3, Hs, Hs), generator=g, device=device), 4).contiguous()
    lib = _lib.load()
    plan = model._plan_for(lr)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    Hp, Wp = plan.query("padded_h") * 4, plan.query("padded_w") * 4
    pre = plan.ws_tensor("srpre", dtype=torch.float32).view(B, 3, Hp, Wp)[..., :Hs, :Hs]
    hr = (pre.clamp(0.0, 1.0) + 0.05 * torch.randn(pre.shape, generator=g, device=device)).clamp(0.0, 1.0).contiguous()

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    for k in ARMS[:2]:
        timed(lambda: arms[k].step(lr, hr), max(1, args.warmup))
    ms = {k: [] for k in ARMS}
    for _ in range(args.repeats):
        for k in ARMS:
            ms[k].append(timed(lambda: arms[k].step(lr, hr), args.steps))

    # the term's kernels alone: a forward and a materialised seed stay valid across the loss calls
    out = torch.zeros(1, device=device)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(lr), None, 1.0, 1, ws, st), "m2t_forward")
    _lib.check(lib.m2t_l1_loss(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), 1.0, _lib.ptr(out), ws, st), "m2t_l1_loss")
    vws = tower.workspace(B, Hs, Hs, True)

    def term_call():
        _lib.check(lib.m2t_vgg_loss(plan.handle, tower.handle, _lib.ptr(hr), args.lambda_perceptual, float(B), 1.0, tower.kind, tower.param,
                                    tower.tap_weights(), _lib.ptr(out), 0, _lib.ptr(vws), ws, st), "m2t_vgg_loss")

    timed(term_call, 1)
    term_ms = [timed(term_call, args.kernel_reps) for _ in range(args.repeats)]

    # resize=True through the module (bicubic to 224 x 224, the tower, and back)
    small = PerceptualLoss(resize=True, device=device).load_vgg_state_dict(sd)
    sr = pre.clamp(0.0, 1.0).contiguous()

    def resize_call():
        leaf = sr.detach().requires_grad_(True)
        small(leaf, hr).backward()

    timed(resize_call, 1)
    resize_ms = [timed(resize_call, args.kernel_reps) for _ in range(args.repeats)]
    del small

    # every MFMA layer at its full-size shape
    layers = []
    for l in range(1, 13):
        ci, co, side = cin[l], _lib.VGG_CHANNELS[l], Hs >> _lib.VGG_LEVEL[l]
        a = torch.randn(B, side, side, ci, device=device).to(torch.bfloat16)
        o = torch.empty(B, side, side, co, device=device, dtype=torch.bfloat16)
        gi = torch.empty_like(a)
        fwd = lambda: _lib.check(lib.m2t_vgg_conv_forward(tower.handle, l, _lib.ptr(a), _lib.ptr(o), B, side, side, 1.0, st), "conv_forward")
        bwd = lambda: _lib.check(lib.m2t_vgg_conv_backward(tower.handle, l, _lib.ptr(o), _lib.ptr(a), _lib.ptr(gi), B, side, side, 1.0, st),
                                 "conv_backward")
        flop = 2.0 * 9 * ci * co * side * side * B
        row = {"layer": l, "cin": ci, "cout": co, "side": side}
        for name, fn in (("forward", fwd), ("backward", bwd)):
            timed(fn, 1)
            t = statistics.median([timed(fn, args.kernel_reps) for _ in range(3)])
            row[name + "_ms"] = round(t, 4)
            row[name + "_tflops"] = round(flop / (t * 1e-3) / 1e12, 1)
        layers.append(row)
        del a, o, gi
    print(json.dumps(result(args, ms, term_ms, resize_ms, layers)))


if __name__ == "__main__":
    main()
