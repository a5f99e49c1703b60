"""What parameter groups and frozen tensors cost -- and save -- at BASELINE.json configs[1]'s geometry (x4, 8 blocks, 128^2 LR, batch 16).

Kernel arms, on the model's own 3 629 760-element flat buffers, every arm alternating with m2t_adam_step_ex in the same process
(clip record off, decoupled decay, EMA: the same nine arrays of traffic):
  * ``aa``          m2t_adam_step_ex against itself: the spread every other comparison is read against
  * ``one_group``   m2t_adam_step_groups with ONE group covering everything
  * ``no_decay``    the real three-group table of the 8-block model (head at a tenth of the rate, no decay on biases and
                    relative-position tables, the tail at twice the rate, the rest by default)
  * ``frozen_body`` the body frozen: about 99 % of the elements are never touched
  * ``launch_floor`` the same entry on 2 048 elements, one group: what a launch of this kernel costs when it moves nothing
Step arms (``TrainStep.step``, track_grad_norm on in every arm so that all of them run a norm pass and an m2t_adam_step_ex-class
pass): ``full`` (no groups), ``tail_only`` (head and body frozen), ``last_block_and_tail`` (head and every block but the last frozen).

Every arm is warmed up first; every repeat is timed with device events.  Prints one JSON line.  Needs a device: without one it fails.

    python tools/param_groups_timing.py [--repeats 5] [--launches 50] [--steps 10] [--warmup 3] [--dtype bf16] [--skip-steps]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NO_DECAY = ["*.bias", "*.rel_h", "*.rel_w"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats of every pair of arms (at least 5)")
    ap.add_argument("--launches", type=int, default=50, help="optimizer launches per timed kernel repeat")
    ap.add_argument("--steps", type=int, default=10, help="training steps per timed step repeat")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--skip-steps", action="store_true", help="kernel arms only")
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats must be at least 5 (the A/A spread is the margin of the comparison)")
    if min(args.launches, args.steps, args.batch, args.blocks, args.lr_size) < 1 or args.warmup < 0:
        ap.error("counts must be positive")
    return args


def no_decay_spec(names):
    """The three-group no-decay recipe by name (the head's and the tail's weights: their biases belong to the no-decay group)."""
    return [{"params": ["head.weight"], "lr_scale": 0.1}, {"params": NO_DECAY, "weight_decay": 0.0},
            {"params": [n for n in names if n.startswith("tail.") and n.endswith(".weight")], "lr_scale": 2.0}]


def frozen_spec(kind: str, n_blocks: int):
    if kind == "frozen_body":
        return [{"params": ["body"], "frozen": True}]
    if kind == "tail_only":
        return [{"params": ["head", "body"], "frozen": True}]
    if kind == "last_block_and_tail":
        return [{"params": ["head"] + [f"body.{b}" for b in range(n_blocks - 1)], "frozen": True}] if n_blocks > 1 else \
               [{"params": ["head"], "frozen": True}]
    raise ValueError(kind)


def summary(ref_ms, arm_ms):
    """Medians, the arm over its reference, and the reference's own repeat-to-repeat spread."""
    r, a = statistics.median(ref_ms), statistics.median(arm_ms)
    return {"ref_ms": round(r, 5), "arm_ms": round(a, 5), "ratio": round(a / r, 4),
            "ref_spread": round((max(ref_ms) - min(ref_ms)) / r, 4),
            "ref_repeats": [round(v, 5) for v in ref_ms], "arm_repeats": [round(v, 5) for v in arm_ms]}


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("param_groups_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.param_groups import resolve_param_groups
    from m2trans_amd.train_step import TrainStep
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=args.blocks, colors=3, compute_dtype=args.dtype)
    lib = _lib.load()
    probe = create_model(margs)
    names = list(probe._names)
    n = probe.flat_params.numel()
    g0 = torch.Generator(device=device).manual_seed(1)
    p, m, e = (torch.randn(n, generator=g0, device=device) for _ in range(3))
    gr = torch.randn(n, generator=g0, device=device) * 0.01
    v = torch.rand(n, generator=g0, device=device) * 1e-4
    lr, wd, b1, b2, eps, ema_d = 1e-4, 1e-2, 0.9, 0.999, 1e-8, 0.999
    st = lambda: _lib.stream_ptr()

    def ex():
        _lib.check(lib.m2t_adam_step_ex(_lib.ptr(p), _lib.ptr(gr), _lib.ptr(m), _lib.ptr(v), n, lr, b1, b2, eps, 1, 1.0, _lib.ptr(e), wd, 1,
                                        ema_d, None, st()), "m2t_adam_step_ex")

    def grouped(spec):
        g = resolve_param_groups(probe, spec)
        table = torch.frombuffer(bytearray(g.pack()), dtype=torch.uint8).to(device)
        ng = g.n_groups
        lrs, wds = (C.c_float * ng)(*g.group_lr(lr)), (C.c_float * ng)(*g.group_weight_decay(wd))
        frozen = (C.c_ubyte * ng)(*[1 if f else 0 for f in g.frozen])

        def call():
            _lib.check(lib.m2t_adam_step_groups(_lib.ptr(p), _lib.ptr(gr), _lib.ptr(m), _lib.ptr(v), n, lrs, b1, b2, eps, 1, 1.0,
                                                _lib.ptr(e), wds, 1, ema_d, None, frozen, ng, _lib.ptr(table), g.n_seg, st()),
                       "m2t_adam_step_groups")
        call.keep = (table, lrs, wds, frozen)
        call.groups = g
        return call

    def timed(fn, k):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(k):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / k

    def floor():
        k = 2048
        small = [torch.zeros(k, device=device) for _ in range(5)]
        blob = C.create_string_buffer(int(lib.m2t_group_table_bytes(1)))
        _lib.check(lib.m2t_group_table_pack((C.c_longlong * 2)(0, k), (C.c_int * 1)(0), 1, k, 1, C.cast(blob, C.c_void_p)),
                   "m2t_group_table_pack")
        table = torch.frombuffer(bytearray(blob.raw), dtype=torch.uint8).to(device)
        lrs, wds, frozen = (C.c_float * 1)(lr), (C.c_float * 1)(wd), (C.c_ubyte * 1)(0)

        def call():
            _lib.check(lib.m2t_adam_step_groups(*[_lib.ptr(t) for t in small[:4]], k, lrs, b1, b2, eps, 1, 1.0, _lib.ptr(small[4]), wds, 1,
                                                ema_d, None, frozen, 1, _lib.ptr(table), 1, st()), "m2t_adam_step_groups")
        call.keep = (small, table, lrs, wds, frozen)
        call.groups = None
        return call

    arms = {"aa": ex, "launch_floor": floor(), "one_group": grouped([{"params": ["head", "body", "tail"]}]), "no_decay": grouped(no_decay_spec(names)),
            "frozen_body": grouped(frozen_spec("frozen_body", args.blocks))}
    kernel = {}
    for name, fn in arms.items():
        timed(ex, max(1, args.warmup))
        timed(fn, max(1, args.warmup))
        ref_ms, arm_ms = [], []
        for _ in range(args.repeats):
            ref_ms.append(timed(ex, args.launches))
            arm_ms.append(timed(fn, args.launches))
        kernel[name] = summary(ref_ms, arm_ms)
        if name not in ("aa", "launch_floor"):
            kernel[name]["n_seg"] = fn.groups.n_seg
            kernel[name]["n_groups"] = fn.groups.n_groups
            kernel[name]["frozen_share"] = round(sum(fn.groups.starts[i + 1] - fn.groups.starts[i] for i, gid in
                                                     enumerate(fn.groups.seg_group) if fn.groups.frozen[gid]) / n, 4)
    out = {"workload": f"x4, {args.blocks} blocks, {args.lr_size}x{args.lr_size} LR, batch {args.batch}: parameter groups in the fused "
                       "optimizer (kernel arms against m2t_adam_step_ex; step arms against the full step)",
           "dtype": args.dtype, "n_params": int(n), "repeats": args.repeats, "launches": args.launches,
           "bytes_per_launch": 9 * 4 * int(n), "kernel_ms": kernel}
    if not args.skip_steps:
        hr = torch.rand((args.batch, 3, args.lr_size * 4, args.lr_size * 4), generator=torch.Generator(device=device).manual_seed(33),
                        device=device)
        x = torch.nn.functional.avg_pool2d(hr, 4).contiguous()
        steps = {"full": TrainStep(create_model(margs).to(device), lr=lr, world_size=1, track_grad_norm=True)}
        for kind in ("tail_only", "last_block_and_tail"):
            steps[kind] = TrainStep(create_model(margs).to(device), lr=lr, world_size=1, track_grad_norm=True,
                                    param_groups=frozen_spec(kind, args.blocks))
        for ts in steps.values():
            timed(lambda: ts.step(x, hr), max(1, args.warmup))
        ms = {k: [] for k in steps}
        for _ in range(args.repeats):
            for k, ts in steps.items():
                ms[k].append(timed(lambda: ts.step(x, hr), args.steps))
        out["steps"] = args.steps
        out["step_ms"] = {k: summary(ms["full"], ms[k]) for k in steps if k != "full"}
        out["step_ms"]["full_ms"] = round(statistics.median(ms["full"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
