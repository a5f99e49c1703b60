"""What local-window InstanceNorm statistics (option "local_norm" of include/m2t.h, `M2Trans.local_norm`) cost: `m2t_forward` on a
plain inference plan against a local-norm plan and against tiled inference, on the same build.

Arms, LR 512 x 512, x4, bf16, B = 1, M2Trans with `--n-blocks` blocks (random weights: time does not depend on them):
    plain          m2t_forward on an inference plan: global statistics over the whole frame;
    plain_again    the same once more: the A/A pair.  "aa_spread" = |median(plain) - median(plain_again)| / median(plain) is what this
                   box cannot tell apart;
    local_96       m2t_forward on a local-norm plan, T = 96 (the training patch): two more launches per block (k_local_norm.hip);
    local_144      the same with T = 144;
    tiled_128_16   `infer.tiled` on inference plans, T = 128, v = 16, tile_batch = 16: the way to training-size statistics before.
"workspace_bytes": of the plain plan, the local-norm plan and the (16, 128, 128) plan tiled inference runs on.
"bytes_per_element_and_block": what the two passes move per element of a feature map, by the segment constants of
m2t_local_norm_tile.h, for both T; "implied_ms" is that over all blocks at the 4.4 TB/s a copy reaches.
"psnr_db": for information only -- local-norm against whole and against tiled on the synthetic tissue image, peak 1.  The weights are
random: this says how far the statistics move the output, not which is better.

Method: every arm is warmed up, then timed with device events around `--reps` back-to-back runs, `--repeats` times; the order of the
arms is reversed on every other repeat; medians are reported with the repeats.  Prints one JSON line and, with `--out`, writes it to
that file as well.  Needs a device: without one it fails.

    python tools/local_norm_timing.py [--reps 5] [--repeats 5] [--n-blocks 8] [--out profiles/local_norm_timing.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ("plain", "plain_again", "local_96", "local_144", "tiled_128_16")
RESULT_KEYS = ("workload", "reps", "repeats", "n_blocks", "ms", "aa_spread", "over_plain", "workspace_bytes",
               "bytes_per_element_and_block", "psnr_db")
TILE, OVERLAP, TILE_BATCH = 128, 16, 16
SEGX, SEGY = 32, 64                   # m2t_local_norm_tile.h
STREAM_BYTES_PER_S = 4.4e12           # what a device-to-device copy reaches


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="runs of an arm per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=8)
    ap.add_argument("--lr", type=int, default=512, help="side of the LR frame")
    ap.add_argument("--scale", type=int, default=4, choices=(2, 3, 4))
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--out", default=None, metavar="FILE", help="also write the JSON line there")
    args = ap.parse_args(argv)
    if min(args.reps, args.n_blocks) < 1 or args.repeats < 2 or args.lr < 32:
        ap.error("--reps and --n-blocks must be positive, --repeats at least 2, --lr at least 32")
    return args


def pass_bytes(T: int, side: int, es: int) -> dict:
    """Bytes per element of a feature map and block.  Pass 1 reads (k + 2 SEGX) / SEGX values of x per output (neighbouring lanes share
    them through the caches: `x_reads_nominal`) and writes one fp64 pair; pass 2 reads (k + 2 SEGY) / SEGY pairs, x once, writes xn."""
    k = min(T, side)
    p1r, p1w = (k + 2 * min(SEGX, side)) / min(SEGX, side) * es, 16.0
    p2r, p2w = (k + 2 * min(SEGY, side)) / min(SEGY, side) * 16.0 + es, float(es)
    return {"pass1_x_reads_nominal": round(p1r, 2), "pass1_write": p1w, "pass2_read": round(p2r, 2), "pass2_write": p2w,
            "total_beyond_cache": round(es + p1w + p2r + p2w, 2)}


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


def psnr(a, b) -> float:
    return round(-10.0 * math.log10(max(float(((a - b).double() ** 2).mean()), 1e-30)), 2)


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("local_norm_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import infer
    from m2trans_amd.M2Trans_network import Plan, create_model
    from tests.gpu_util import make_args, smooth_hr
    torch.manual_seed(34)
    side, s, nb = args.lr, args.scale, args.n_blocks
    model = create_model(make_args(s, nb, args.dtype)).to("cuda").eval()
    model.lean_inference()
    lr = smooth_hr(1, side, 7, device="cuda").contiguous()
    dt = model._dtype_code()
    plans = {"plain": Plan(1, side, side, s, nb, dt, lr.device, inference=True),
             "local_96": Plan(1, side, side, s, nb, dt, lr.device, inference=True, local_norm=96),
             "local_144": Plan(1, side, side, s, nb, dt, lr.device, inference=True, local_norm=144)}
    run = lambda k: model._run_forward(plans[k], lr, keep=False)
    tiled = lambda: infer.tiled(model, lr, TILE, OVERLAP, TILE_BATCH)
    with torch.no_grad():
        whole, l96, l144, til = run("plain"), run("local_96"), run("local_144"), tiled()
        assert all(bool(torch.isfinite(t).all()) for t in (whole, l96, l144, til))
        psnr_db = {"local_96_vs_whole": psnr(l96, whole), "local_96_vs_tiled": psnr(l96, til), "local_144_vs_whole": psnr(l144, whole),
                   "local_144_vs_tiled": psnr(l144, til), "tiled_vs_whole": psnr(til, whole)}
        del whole, l96, l144, til
        ms = alternate({"plain": lambda: run("plain"), "plain_again": lambda: run("plain"), "local_96": lambda: run("local_96"),
                        "local_144": lambda: run("local_144"), "tiled_128_16": tiled}, args.reps, args.repeats)
    assert tuple(ms) == ARMS
    med = {k: statistics.median(v) for k, v in ms.items()}
    es = 2 if args.dtype == "bf16" else 4
    elems = side * side * 64
    bpe = {}
    for T in (96, 144):
        b = pass_bytes(T, side, es)
        b["implied_ms"] = round(b["total_beyond_cache"] * elems * nb / STREAM_BYTES_PER_S * 1e3, 4)
        b["measured_extra_ms"] = round(med[f"local_{T}"] - med["plain"], 4)
        bpe[f"T={T}"] = b
    tile_plan = [k for k in model._plans if k[0] == TILE_BATCH]
    out = {"workload": f"m2t_forward of M2Trans x{s} {args.dtype} at LR {side}x{side}, B=1, {nb} blocks: a plain inference plan (twice), local-norm "
                       f"plans T=96 and T=144, infer.tiled (T={TILE}, v={OVERLAP}, tile_batch={TILE_BATCH}) on inference plans",
           "reps": args.reps, "repeats": args.repeats, "n_blocks": nb,
           "ms": {k: {"median": round(med[k], 4), "repeats": [round(t, 4) for t in v]} for k, v in ms.items()},
           "aa_spread": round(abs(med["plain"] - med["plain_again"]) / med["plain"], 4),
           "over_plain": {k: round(med[k] / med["plain"], 4) for k in ARMS[2:]},
           "workspace_bytes": {"plain": plans["plain"].query("workspace_bytes"), "local_norm": plans["local_96"].query("workspace_bytes"),
                               "tiles_16x128x128": model._plans[tile_plan[0]].query("workspace_bytes") if tile_plan else None},
           "bytes_per_element_and_block": bpe, "psnr_db": psnr_db}
    assert tuple(out) == RESULT_KEYS
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
