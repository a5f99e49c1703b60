"""What the step health record (option "health" of include/m2t.h, `TrainStep(track_health=K)`) costs: the training step of
BASELINE configs[1] (M2Trans x4, bf16, 16 LR patches of 128 x 128, L1) with the option off, with the record on every step, with
K = 50, and the record's launches alone.

Arms, each a TrainStep of its own on the same weights and batch (`--reps` back-to-back steps per timed repeat, so that K = 50
records once per repeat at the default):
    off        no option: the plan is laid out and launched as before;
    off_aa     `off` once more: the A/A pair.  "aa_spread" = |median(off) - median(off_aa)| / median(off) is what this box cannot
               tell apart;
    every      level 2, recorded on every step (track_health = 1);
    k50        level 2, recorded on the steps with step_count % 50 == 0 (track_health = 50);
    switched   the `every` plan with option "health_on" at 0: the layout of the record without its launches.
"record_ms" = median(every) - median(switched): the four launches alone, on the step they ride on.  "record_bytes" is what they read
(every row's elements in its stored type); "copy_ms" is a torch `copy_` of a workspace slice of that many bytes (which also writes
them: the project's usual yardstick for a streaming pass) and "record_over_copy" their ratio.

Method: every arm is warmed up, then timed with device events, `--repeats` times; the order of the arms is reversed on every other
repeat; medians are reported with the repeats.  Prints one JSON line.  Needs a device: without one it fails.

    python tools/health_timing.py [--reps 50] [--repeats 5] [--n-blocks 8] [--batch 16] [--lr 128]
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

ARMS = ("off", "off_aa", "every", "k50", "switched")
RESULT_KEYS = ("workload", "reps", "repeats", "n_blocks", "lr", "step_ms", "aa_spread", "every_over_off", "k50_over_off", "switched_over_off",
               "record_ms", "record_bytes", "record_gb_per_s", "copy_ms", "record_over_copy", "rows", "workspace_bytes")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="steps per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr", type=int, default=128, help="LR patch side")
    args = ap.parse_args(argv)
    if min(args.reps, args.repeats, args.n_blocks, args.batch) < 1 or args.repeats < 2 or args.lr < 32:
        ap.error("counts must be positive, repeats >= 2, lr >= 32")
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


def record_bytes(plan) -> int:
    """Bytes the record's launches read: every row's elements in the type they are stored in (names from the library)."""
    from m2trans_amd import _lib
    lib, es, total = _lib.load(), (4 if plan.dtype == _lib.F32 else 2), 0
    for i in range(plan.query("health_rows")):
        plan.query(f"health_name:{i}")
        name = lib.m2t_last_error_string().decode()
        if name == "sr":
            total += 4 * plan.B * 3 * plan.H0 * plan.W0 * plan.scale ** 2
        elif name == "grads":
            total += 4 * plan.query("num_params")
        else:
            f32 = name == "srpre" or name.endswith((".mean", ".rstd"))
            total += plan.query("wsn:" + name) * (4 if f32 else es)
    return total


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("health_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.train_step import TrainStep
    from tests.gpu_util import make_args
    B, L = args.batch, args.lr
    torch.manual_seed(33)
    first = create_model(make_args(4, args.n_blocks, "bf16")).to("cuda")
    state = {k: v.clone() for k, v in first.state_dict().items()}
    x, hr = torch.rand(B, 3, L, L, device="cuda"), torch.rand(B, 3, 4 * L, 4 * L, device="cuda")
    steps, models = {}, {}
    for arm, K in (("off", 0), ("every", 1), ("k50", 50)):
        m = create_model(make_args(4, args.n_blocks, "bf16")).to("cuda")
        torch.nn.Module.load_state_dict(m, state, strict=True)
        steps[arm], models[arm] = TrainStep(m, lr=1e-5, world_size=1, track_health=K), m
        steps[arm].step(x, hr)
    torch.cuda.synchronize()
    every_plan = steps["every"]._last_plan

    def switched():
        ts = steps["every"]
        K, ts.track_health = ts.track_health, 1 << 62      # (no step number but 0 is a multiple: the switch goes to 0 and stays there)
        ts.step(x, hr)
        ts.track_health = K
    variants = {"off": lambda: steps["off"].step(x, hr), "every": lambda: steps["every"].step(x, hr), "k50": lambda: steps["k50"].step(x, hr),
                "switched": switched, "off_aa": lambda: steps["off"].step(x, hr)}
    ms = alternate(variants, args.reps, args.repeats)
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = record_bytes(every_plan)
    src = every_plan.workspace[:nbytes]
    dst = torch.empty_like(src)
    copy_ms = statistics.median(alternate({"copy": lambda: dst.copy_(src)}, 20, args.repeats)["copy"])
    rec_ms = med["every"] - med["switched"]
    out = {"workload": "TrainStep.step of M2Trans x4 bf16 (BASELINE configs[1]): option \"health\" off / level 2 on every step / every "
                       "50th step / laid out but switched off; off_aa: the first arm again",
           "reps": args.reps, "repeats": args.repeats, "n_blocks": args.n_blocks, "lr": [B, 3, L, L],
           "step_ms": {k: {"median": round(med[k], 4), "repeats": [round(t, 4) for t in ms[k]]} for k in ARMS},
           "aa_spread": round(abs(med["off"] - med["off_aa"]) / med["off"], 4),
           "every_over_off": round(med["every"] / med["off"], 4), "k50_over_off": round(med["k50"] / med["off"], 4),
           "switched_over_off": round(med["switched"] / med["off"], 4),
           "record_ms": round(rec_ms, 4), "record_bytes": nbytes,
           "record_gb_per_s": round(nbytes / 1e6 / rec_ms, 1) if rec_ms > 0 else None, "copy_ms": round(copy_ms, 4),
           "record_over_copy": round(rec_ms / copy_ms, 3) if copy_ms > 0 else None, "rows": every_plan.query("health_rows"),
           "workspace_bytes": {"off": steps["off"]._last_plan.query("workspace_bytes"), "every": every_plan.query("workspace_bytes")}}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
