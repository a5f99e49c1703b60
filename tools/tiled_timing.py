"""What tiled inference costs (m2trans_amd/infer.py, k_tiles.hip), what it saves in workspace, and how close its two kernels come to a
plain copy.

Model arms, LR 512 x 512, x4, bf16, B = 1, M2Trans with `--n-blocks` blocks (random weights: time does not depend on them):
    whole     one forward on the whole image: a (1, 512, 512) plan;
    tiled     `infer.tiled`, T = 128, v = 16, tile_batch = 16: 5 x 5 = 25 tiles in chunks of 16 and 9 (m2t_tile_gather, the forward, the
              copy into the SR-tile buffer), then one m2t_tile_blend;
    tiled_aa  tiled once more: the A/A pair.  "aa_spread" = |median(tiled) - median(tiled_aa)| / median(tiled) is what this box cannot
              tell apart; a difference between two arms below it is no difference.
    chunk_copy  the per-chunk copies into the SR-tile buffer alone: the price of not letting the model write into that buffer.
"prices": what is deliberately not built.  "chunk_copy_ms" per image (above); "gather_then_pack_us" against "pack_alone_us" for one
chunk of `Tiled(SelfEnsemble(model))` (2 tiles -> 16 views): their difference is the most a fused gather + 8-view pack could save per
chunk.
Kernels alone, at the same shape: the gather of all 25 tiles ([25,3,128,128] written), the blend without and with the seam
([1,3,2048,2048] written once or twice), each against a torch device-to-device `copy_` of the bytes the kernel WRITES.  "copy_ratio" =
the copy's time over the kernel's.  The blend reads more than it writes wherever tiles overlap (here 25 x 512^2 read for 2048^2
written: 1.56 x), so its ratio is reported and not gated.
"workspace_bytes": the plan workspace of (1, 512, 512) and of (16, 128, 128), a host query without a device allocation.
"psnr_tiled_vs_whole_db": between the two outputs on the synthetic tissue image, peak 1; the weights are random, so this says how far
the tiles' statistics move the output, not which is better.

Method: every arm is warmed up, then timed with device events around `--reps` back-to-back runs, `--repeats` times; the order of the
arms is reversed on every other repeat; medians are reported with the repeats.  Prints one JSON line.  Needs a device: without one it
fails.

    python tools/tiled_timing.py [--reps 5] [--kernel-reps 50] [--repeats 5] [--n-blocks 8]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESULT_KEYS = ("workload", "reps", "kernel_reps", "repeats", "n_blocks", "model_ms", "aa_spread", "kernels", "prices", "workspace_bytes",
               "psnr_tiled_vs_whole_db")
SIDE, SCALE, TILE, OVERLAP, TILE_BATCH = 512, 4, 128, 16, 16


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="runs of a model arm per timed repeat")
    ap.add_argument("--kernel-reps", type=int, default=50, help="launches of a kernel per timed repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=8)
    args = ap.parse_args(argv)
    if min(args.reps, args.kernel_reps, args.repeats, args.n_blocks) < 1:
        ap.error("counts must be positive")
    return args


def written_bytes(kind: str, n_tiles: int, tile: int, side: int, scale: int) -> int:
    """Bytes a launch writes: the gather its LR tiles, the blend the SR image, once more with the seam."""
    return {"gather": n_tiles * 3 * tile * tile, "blend": 3 * (side * scale) ** 2, "blend_seam": 2 * 3 * (side * scale) ** 2}[kind] * 4


def workspace_bytes(B: int, H: int, W: int, scale: int, n_blocks: int, dtype: int) -> int:
    """The workspace a (B, H, W) plan asks for: a host query, nothing is allocated on a device."""
    from m2trans_amd import _lib
    lib, h = _lib.load(), C.c_void_p()
    _lib.check(lib.m2t_plan_create(C.byref(h), B, H, W, scale, n_blocks, dtype), "m2t_plan_create")
    try:
        return int(lib.m2t_plan_query(h, b"workspace_bytes"))
    finally:
        lib.m2t_plan_destroy(h)


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
        raise SystemExit("tiled_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib, infer
    from m2trans_amd.M2Trans_network import create_model
    from tests.gpu_util import make_args, smooth_hr
    lib, st = _lib.load(), _lib.stream_ptr()
    torch.manual_seed(34)
    model = create_model(make_args(SCALE, args.n_blocks, "bf16")).to("cuda").eval()
    lr = smooth_hr(1, SIDE, 7, device="cuda").contiguous()
    n_tiles = len(infer.tile_grid(SIDE, TILE, OVERLAP)[1]) ** 2
    sr_side, sr_tile = SIDE * SCALE, TILE * SCALE

    with torch.no_grad():
        whole = model(lr)
        tiled = infer.tiled(model, lr, TILE, OVERLAP, TILE_BATCH)
        assert bool(torch.isfinite(whole).all()) and bool(torch.isfinite(tiled).all()) and tiled.shape == whole.shape
        psnr = -10.0 * math.log10(max(float(((tiled - whole).double() ** 2).mean()), 1e-30))
        del whole, tiled
        chunk = torch.rand(TILE_BATCH, 3, sr_tile, sr_tile, device="cuda")
        last = torch.rand(n_tiles - TILE_BATCH, 3, sr_tile, sr_tile, device="cuda")
        buf = torch.empty(n_tiles, 3, sr_tile, sr_tile, device="cuda")

        def chunk_copy():
            buf[:TILE_BATCH].copy_(chunk)
            buf[TILE_BATCH:].copy_(last)

        model_ms = alternate({"whole": lambda: model(lr), "tiled": lambda: infer.tiled(model, lr, TILE, OVERLAP, TILE_BATCH),
                              "tiled_aa": lambda: infer.tiled(model, lr, TILE, OVERLAP, TILE_BATCH), "chunk_copy": chunk_copy},
                             args.reps, args.repeats)
    med = {k: statistics.median(v) for k, v in model_ms.items()}
    del model, chunk, last

    tiles_lr = torch.empty(n_tiles, 3, TILE, TILE, device="cuda")
    buf.uniform_()
    image, seam = torch.empty(1, 3, sr_side, sr_side, device="cuda"), torch.empty(1, 3, sr_side, sr_side, device="cuda")
    launches = {
        "gather": lambda: _lib.check(lib.m2t_tile_gather(lr.data_ptr(), 1, 3, SIDE, SIDE, TILE, OVERLAP, 0, n_tiles, tiles_lr.data_ptr(), st)),
        "blend": lambda: _lib.check(lib.m2t_tile_blend(buf.data_ptr(), 1, 3, SIDE, SIDE, TILE, OVERLAP, SCALE, image.data_ptr(), None, st)),
        "blend_seam": lambda: _lib.check(lib.m2t_tile_blend(buf.data_ptr(), 1, 3, SIDE, SIDE, TILE, OVERLAP, SCALE, image.data_ptr(),
                                                            seam.data_ptr(), st)),
    }
    variants, nbytes = {}, {}
    for kind, fn in launches.items():
        nbytes[kind] = written_bytes(kind, n_tiles, TILE, SIDE, SCALE)
        src = torch.rand(nbytes[kind] // 4, device="cuda")                          # the bytes the kernel writes, as float32
        dst = torch.empty_like(src)
        variants[kind] = fn
        variants[kind + "_copy"] = (lambda d=dst, s_=src: d.copy_(s_))
    two = infer.tile_gather(lr, TILE, OVERLAP, 0, 2)
    variants["gather_then_pack"] = lambda: infer._pack(infer.tile_gather(lr, TILE, OVERLAP, 0, 2))
    variants["pack_alone"] = lambda: infer._pack(two)
    ms = alternate(variants, args.kernel_reps, args.repeats)
    kernels = {}
    for kind in launches:
        t, tc = statistics.median(ms[kind]), statistics.median(ms[kind + "_copy"])
        kernels[kind] = {"bytes_written": nbytes[kind], "us": round(t * 1e3, 3), "us_repeats": [round(v * 1e3, 3) for v in ms[kind]],
                         "written_bytes_per_s": round(nbytes[kind] / (t * 1e-3), 1), "copy_us": round(tc * 1e3, 3),
                         "copy_us_repeats": [round(v * 1e3, 3) for v in ms[kind + "_copy"]], "copy_ratio": round(tc / t, 4)}

    out = {"workload": f"tiled inference of M2Trans x{SCALE} bf16 at LR {SIDE}x{SIDE}, B=1: whole-image forward, infer.tiled (T={TILE}, v={OVERLAP}, "
                       f"tile_batch={TILE_BATCH}: {n_tiles} tiles; tiled_aa: the same again), the per-chunk copies alone; gather / blend kernels "
                       "against a torch copy_ of the bytes they write",
           "reps": args.reps, "kernel_reps": args.kernel_reps, "repeats": args.repeats, "n_blocks": args.n_blocks,
           "model_ms": summarise(model_ms), "aa_spread": round(abs(med["tiled"] - med["tiled_aa"]) / med["tiled"], 4), "kernels": kernels,
           "prices": {"chunk_copy_ms": round(med["chunk_copy"], 4),
                      "gather_then_pack_us": round(statistics.median(ms["gather_then_pack"]) * 1e3, 3),
                      "pack_alone_us": round(statistics.median(ms["pack_alone"]) * 1e3, 3)},
           "workspace_bytes": {"whole_1x512x512": workspace_bytes(1, SIDE, SIDE, SCALE, args.n_blocks, _lib.BF16),
                               "tiles_16x128x128": workspace_bytes(TILE_BATCH, TILE, TILE, SCALE, args.n_blocks, _lib.BF16)},
           "psnr_tiled_vs_whole_db": round(psnr, 2)}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
