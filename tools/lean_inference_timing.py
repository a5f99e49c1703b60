"""What an inference plan (option "inference" of include/m2t.h, `M2Trans.lean_inference`) saves and costs: forward time and
`workspace_bytes` of the training layout against the inference layout, on the same build.

Per shape, M2Trans x4 with `--n-blocks` blocks (random weights: time does not depend on them), one plan of each layout:
    train      m2t_forward on a training plan (every activation, gelu' and q | k | v store of the training step);
    lean       m2t_forward on an inference plan (the same kernels in the same order; X1.. rotate through two buffers, one set of
               per-block regions, null pointers for what only the backward pass reads);
    train_aa   `train` once more: the A/A pair.  "aa_spread" = |median(train) - median(train_aa)| / median(train) is what this box
               cannot tell apart; a difference between `train` and `lean` below it is no difference.
Shapes: LR 128 x 128, B = 16 (the training batch); LR 512 x 512, B = 1 (a whole frame); LR 256 x 256, B = 8 (the x8 self-ensemble
batch of one frame), all in bf16; and fp32 at the first shape.  The outputs of both layouts are compared for equality first.

Method: every variant is warmed up, then timed with device events around `--reps` back-to-back forwards, `--repeats` times; the
order of the variants is reversed on every other repeat; medians are reported with the repeats.  Prints one JSON line.  Needs a
device: without one it fails.

    python tools/lean_inference_timing.py [--reps 10] [--repeats 5] [--n-blocks 8]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESULT_KEYS = ("workload", "reps", "repeats", "n_blocks", "shapes")
SHAPES = (("bf16", 16, 128, 128), ("bf16", 1, 512, 512), ("bf16", 8, 256, 256), ("fp32", 16, 128, 128))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="forwards per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=8)
    args = ap.parse_args(argv)
    if min(args.reps, args.repeats, args.n_blocks) < 1:
        ap.error("counts must be positive")
    return args


def timed(fn, n: int) -> float:
    """Milliseconds per run of fn over n back-to-back runs, by device events."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


def alternate(variants: dict, reps: int, repeats: int) -> dict:
    """{name: [ms per run, one per repeat]}; the order of the variants is reversed on every other repeat."""
    for fn in variants.values():
        timed(fn, min(reps, 3))
    out = {k: [] for k in variants}
    for r in range(repeats):
        for k in (list(variants) if r % 2 == 0 else list(reversed(variants))):
            out[k].append(timed(variants[k], reps))
    return out


def measure_shape(dtype: str, B: int, H: int, W: int, n_blocks: int, reps: int, repeats: int) -> dict:
    import torch
    from m2trans_amd.M2Trans_network import Plan, create_model
    from tests.gpu_util import make_args
    torch.manual_seed(33)
    model = create_model(make_args(4, n_blocks, dtype)).to("cuda").eval()
    x = torch.rand(B, 3, H, W, device="cuda")
    plans = {k: Plan(B, H, W, 4, n_blocks, model._dtype_code(), x.device, inference=(k == "lean")) for k in ("train", "lean")}
    run = lambda k: model._run_forward(plans[k], x, keep=False)
    equal = bool(torch.equal(run("train"), run("lean")))
    ms = alternate({"train": lambda: run("train"), "lean": lambda: run("lean"), "train_aa": lambda: run("train")}, reps, repeats)
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = {k: plans[k].query("workspace_bytes") for k in plans}
    return {"dtype": dtype, "lr": [B, 3, H, W], "sr_equal": equal,
            "forward_ms": {k: {"median": round(med[k], 4), "repeats": [round(t, 4) for t in v]} for k, v in ms.items()},
            "aa_spread": round(abs(med["train"] - med["train_aa"]) / med["train"], 4),
            "lean_over_train": round(med["lean"] / med["train"], 4),
            "workspace_bytes": nbytes, "bytes_ratio": round(nbytes["lean"] / nbytes["train"], 4)}


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lean_inference_timing.py needs a HIP device: nothing is measured without one")
    shapes = []
    with torch.no_grad():
        for dtype, B, H, W in SHAPES:
            shapes.append(measure_shape(dtype, B, H, W, args.n_blocks, args.reps, args.repeats))
            torch.cuda.empty_cache()
    out = {"workload": "m2t_forward of M2Trans x4 on a training plan against an inference plan (option \"inference\"): the same kernels "
                       "in the same order on a forward-only workspace; train_aa: the training plan again",
           "reps": args.reps, "repeats": args.repeats, "n_blocks": args.n_blocks, "shapes": shapes}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
