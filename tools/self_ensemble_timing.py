"""What geometric self-ensemble costs (m2trans_amd/infer.py, k_infer.hip), and how close its two kernels come to a plain copy.

Model variants, LR 128 x 128, x4, bf16, B = 1, M2Trans with `--n-blocks` blocks (random weights: time does not depend on them):
    a  one plain forward (no ensemble: the floor);
    b  eight batch-1 forwards, the views, inverses and the mean with torch operations;
    c  one batch-8 forward, pack and merge with torch operations (tests/infer_ref.py);
    d  `infer.self_ensemble`: m2t_dihedral_pack, one batch-8 forward, m2t_dihedral_merge;
    d_aa  d once more: the A/A pair.  "aa_spread" = |median(d) - median(d_aa)| / median(d) is what this box cannot tell apart; a
       difference between two variants below it is no difference.
Kernels alone: pack at [3,128,128] and [48,512,512], merge with and without spread at [3,512,512] and [48,512,512], and a torch
device-to-device `copy_` that moves the same number of bytes (read + written: pack 9 x planes H W 4 B, merge 9 x or 10 x that; the
copy is of half as many bytes, read once and written once).  "bytes_per_s" = those bytes over the time per launch, the traffic the
algorithm needs, not a counter; "copy_ratio" = the kernel's rate over the copy's.  The large shape moves 453 MB per launch, more than
the Infinity Cache holds; the small ones stay in cache and are launch-bound, named as such.

Method: every variant is warmed up, then timed with device events around `--reps` back-to-back runs, `--repeats` times; the order
of the variants is reversed on every other repeat; medians are reported with the repeats.  Prints one JSON line.  Needs a device:
without one it fails.

    python tools/self_ensemble_timing.py [--reps 20] [--kernel-reps 50] [--repeats 5] [--n-blocks 8]
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

RESULT_KEYS = ("workload", "reps", "kernel_reps", "repeats", "n_blocks", "model_ms", "aa_spread", "kernels")
SMALL, LARGE = (3, 128, 128, 4), (48, 512, 512, 1)             # (planes, H, W, scale of the merge's side)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="runs of a model variant per timed repeat")
    ap.add_argument("--kernel-reps", type=int, default=50, help="launches of a kernel per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=8)
    args = ap.parse_args(argv)
    if min(args.reps, args.kernel_reps, args.repeats, args.n_blocks) < 1:
        ap.error("counts must be positive")
    return args


def moved_bytes(kind: str, planes: int, H: int, W: int) -> int:
    """Bytes a launch has to move: pack reads 1 and writes 8 planes' worth, merge reads 8 and writes 1 (mean) or 2 (with spread)."""
    return {"pack": 9, "merge": 9, "merge_spread": 10}[kind] * planes * H * W * 4


def summarise(times: dict) -> dict:
    return {k: {"median": round(statistics.median(v), 4), "repeats": [round(t, 4) for t in v]} for k, v in times.items()}


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


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("self_ensemble_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib, infer
    from m2trans_amd.M2Trans_network import create_model
    from tests import infer_ref as R
    from tests.gpu_util import make_args
    lib, st = _lib.load(), _lib.stream_ptr()
    torch.manual_seed(33)
    model = create_model(make_args(4, args.n_blocks, "bf16")).to("cuda").eval()
    lr = torch.rand(1, 3, 128, 128, device="cuda")

    def b_eight_forwards():
        outs = [R.inverse(model(R.view(lr, k)), k) for k in range(8)]
        return torch.stack(outs).mean(dim=0)

    def c_torch_batch():
        a, b = R.pack(lr)
        out = model(torch.cat([a, b]))
        return torch.stack(R.unpack(out[:4], out[4:])).mean(dim=0)

    with torch.no_grad():
        d = infer.self_ensemble(model, lr)
        assert bool(torch.isfinite(d).all()) and float((c_torch_batch() - d).abs().max()) <= 1e-5 * (1.0 + float(d.abs().max()))
        model_ms = alternate({"a": lambda: model(lr), "b": b_eight_forwards, "c": c_torch_batch,
                              "d": lambda: infer.self_ensemble(model, lr), "d_aa": lambda: infer.self_ensemble(model, lr)},
                             args.reps, args.repeats)
    med = {k: statistics.median(v) for k, v in model_ms.items()}
    del model

    kernels = {}
    for tag, (planes, H, W, s) in (("small", SMALL), ("large", LARGE)):
        Hs, Ws = H * s, W * s
        x = torch.rand(planes, H, W, device="cuda")
        pa, pb = torch.empty(4 * planes * H * W, device="cuda"), torch.empty(4 * planes * H * W, device="cuda")
        sa, sb = torch.rand(4, planes, Hs, Ws, device="cuda"), torch.rand(4, planes, Ws, Hs, device="cuda")
        mean, spread = torch.empty(planes, Hs, Ws, device="cuda"), torch.empty(planes, Hs, Ws, device="cuda")
        launches = {
            "pack": ((planes, H, W), lambda: _lib.check(lib.m2t_dihedral_pack(x.data_ptr(), planes, H, W, pa.data_ptr(), pb.data_ptr(), st))),
            "merge": ((planes, Hs, Ws), lambda: _lib.check(lib.m2t_dihedral_merge(sa.data_ptr(), sb.data_ptr(), planes, Hs, Ws, mean.data_ptr(), None, st))),
            "merge_spread": ((planes, Hs, Ws), lambda: _lib.check(lib.m2t_dihedral_merge(sa.data_ptr(), sb.data_ptr(), planes, Hs, Ws, mean.data_ptr(),
                                                                                       spread.data_ptr(), st))),
        }
        variants, nbytes = {}, {}
        for kind, (shape, fn) in launches.items():
            nbytes[kind] = moved_bytes(kind, *shape)
            src = torch.rand(nbytes[kind] // 8, device="cuda")                      # half the bytes, as float32: read once, written once
            dst = torch.empty_like(src)
            variants[kind] = fn
            variants[kind + "_copy"] = (lambda d=dst, s_=src: d.copy_(s_))
        ms = alternate(variants, args.kernel_reps, args.repeats)
        for kind, (shape, _) in launches.items():
            t, tc = statistics.median(ms[kind]), statistics.median(ms[kind + "_copy"])
            kernels[f"{kind}_{tag}"] = {"shape": list(shape), "bytes": nbytes[kind], "us": round(t * 1e3, 3), "us_repeats": [round(v * 1e3, 3) for v in ms[kind]],
                                        "bytes_per_s": round(nbytes[kind] / (t * 1e-3), 1), "copy_us": round(tc * 1e3, 3),
                                        "copy_us_repeats": [round(v * 1e3, 3) for v in ms[kind + "_copy"]],
                                        "copy_bytes_per_s": round(nbytes[kind] / (tc * 1e-3), 1), "copy_ratio": round(tc / t, 4)}
        del x, pa, pb, sa, sb, mean, spread, variants, launches

    out = {"workload": "geometric self-ensemble of M2Trans x4 bf16 at LR 128x128, B=1: a plain forward, b 8 batch-1 forwards + torch, "
                       "c torch pack/merge + 1 batch-8 forward, d infer.self_ensemble (d_aa: the same again); pack / merge kernels against a "
                       "torch copy_ of the same bytes",
           "reps": args.reps, "kernel_reps": args.kernel_reps, "repeats": args.repeats, "n_blocks": args.n_blocks,
           "model_ms": summarise(model_ms), "aa_spread": round(abs(med["d"] - med["d_aa"]) / med["d"], 4), "kernels": kernels}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
