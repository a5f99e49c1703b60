"""What the TransBlock (util/rlutrans.py) costs on the device, forward and backward: the four C entry points
(include/m2t.h, include/m2t_rlutrans.h) on preallocated buffers, next to the same block written in eager torch ops on the same
device (forward + backward, in the same element type) -- the only yardstick there is: the block has no predecessor.

Arms, per (N, dtype): ``infer`` = m2t_transblock_forward, ``fwd_train`` = m2t_transblock_forward_train, ``bwd`` =
m2t_transblock_backward with gx and gparams, ``bwd_data`` = the same with gparams = NULL, ``eager`` = forward + backward of the torch
block.  The arms alternate inside every repeat, all are warmed up first, every sample is timed with device events around `--calls`
back-to-back calls.  The result also carries the largest ``rel`` = max|a - b| / max|b| of the library's gx and parameter gradients
against the eager ones at the timed size (fp32 eager for both dtypes), so that the times are times of the right numbers.

Prints one JSON line.  Needs a device: without one it fails.

    python tools/transblock_timing.py [--batch 16] [--tokens 2304 4096] [--dtypes fp32 bf16] [--repeats 5] [--calls 20] [--warmup 3]
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

ARMS = ("infer", "fwd_train", "bwd", "bwd_data", "eager")
RESULT_KEYS = ("workload", "batch", "repeats", "calls", "cases")
CASE_KEYS = ("tokens", "dtype", "ms", "ms_repeats", "spread", "train_ms", "eager_over_train", "workspace_mib", "grad_rel_vs_eager_fp32")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--tokens", type=int, nargs="+", default=[2304, 4096])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--repeats", type=int, default=5, help="timed rounds of the five arms (at least 3)")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every arm before the first repeat")
    args = ap.parse_args(argv)
    if args.repeats < 3:
        ap.error("--repeats must be at least 3 (the spread of the repeats is the margin of every comparison)")
    if min(args.batch, args.calls) < 1 or args.warmup < 0 or min(args.tokens) < 16:
        ap.error("--batch and --calls must be positive, --tokens at least 16")
    return args


def case_result(tokens: int, dtype: str, ms: dict, workspace_bytes: int, grad_rel: float):
    """One entry of "cases" from the per-repeat times ms = {arm: [ms per call]}."""
    med = {k: statistics.median(ms[k]) for k in ARMS}
    train = med["fwd_train"] + med["bwd"]
    out = {"tokens": tokens, "dtype": dtype, "ms": {k: round(med[k], 4) for k in ARMS},
           "ms_repeats": {k: [round(v, 4) for v in ms[k]] for k in ARMS},
           "spread": {k: round((max(ms[k]) - min(ms[k])) / med[k], 4) for k in ARMS},
           "train_ms": round(train, 4), "eager_over_train": round(med["eager"] / train, 3),
           "workspace_mib": round(workspace_bytes / 2 ** 20, 1), "grad_rel_vs_eager_fp32": float(f"{grad_rel:.3e}")}
    assert tuple(out) == CASE_KEYS
    return out


def eager_block(x, p):
    """TransBlock.forward in torch ops (the arithmetic of oracle/rlutrans_oracle.py; when 16 divides N the 16 chunks are one batched
    product instead of a Python loop, which is the faster way to write it)."""
    import torch
    import torch.nn.functional as F
    B, N, C = x.shape
    h = F.layer_norm(x, (C,), p["norm1.weight"], p["norm1.bias"], 1e-5)
    h = F.linear(h, p["atten.reduce.weight"])
    qkv = F.linear(h, p["atten.qkv.weight"]).reshape(B, N, 3, 8, 8).permute(2, 0, 3, 1, 4)          # [3, B, heads, N, 8]
    L = N // 16
    if N % 16 == 0:
        q, k, v = (t.reshape(B, 8, 16, L, 8) for t in qkv)
        a = ((q @ k.transpose(-2, -1)) * 8 ** -0.5).softmax(-1) @ v
        a = a.reshape(B, 8, N, 8).transpose(1, 2).reshape(B, N, C)
    else:
        outs = []
        for qc, kc, vc in zip(*(torch.split(t, L, dim=-2) for t in qkv)):
            outs.append((((qc @ kc.transpose(-2, -1)) * 8 ** -0.5).softmax(-1) @ vc).transpose(1, 2))
        a = torch.cat(outs, dim=1).reshape(B, N, C)
    x = x + F.linear(a, p["atten.proj.weight"], p["atten.proj.bias"])
    h = F.layer_norm(x, (C,), p["norm2.weight"], p["norm2.bias"], 1e-5)
    return x + F.linear(F.relu(F.linear(h, p["mlp.fc1.weight"], p["mlp.fc1.bias"])), p["mlp.fc2.weight"], p["mlp.fc2.bias"])


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("transblock_timing.py needs a HIP device: nothing is measured without one")
    from m2trans_amd import _lib
    from m2trans_amd.rlutrans import TransBlock
    device = torch.device("cuda", 0)
    lib = _lib.load()
    torch.manual_seed(33)
    names = list(TransBlock().state_dict().keys())
    params = {k: v.to(device) for k, v in TransBlock().state_dict().items()}
    flat = torch.cat([params[k].reshape(-1).float() for k in names]).contiguous()
    st = _lib.stream_ptr()
    B = args.batch

    def timed(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n

    cases = []
    for N in args.tokens:
        g = torch.Generator(device=device).manual_seed(N)
        x = torch.randn(B, N, 64, generator=g, device=device)
        gy = torch.randn(B, N, 64, generator=g, device=device)
        # fp32 eager gradients: what the library's numbers are compared with at this size
        p32 = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        x32 = x.clone().requires_grad_(True)
        want = torch.autograd.grad(eager_block(x32, p32), [x32] + [p32[k] for k in names], gy)
        want_flat = torch.cat([t.reshape(-1) for t in want[1:]])
        for dtype in args.dtypes:
            code = _lib.F32 if dtype == "fp32" else _lib.BF16
            ws_i = torch.empty(int(lib.m2t_transblock_workspace_bytes(B, N, code)), dtype=torch.uint8, device=device)
            ws_t = torch.empty(int(lib.m2t_transblock_train_workspace_bytes(B, N, code)), dtype=torch.uint8, device=device)
            y, gx, gp = torch.empty_like(x), torch.empty_like(x), torch.empty(_lib.TRANSBLOCK_NPARAMS, device=device)
            tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
            pe = {k: v.to(tdt).requires_grad_(True) for k, v in params.items()}
            xe, gye = x.to(tdt).requires_grad_(True), gy.to(tdt)

            def infer():
                _lib.check(lib.m2t_transblock_forward(_lib.ptr(flat), _lib.ptr(x), _lib.ptr(y), B, N, code, _lib.ptr(ws_i), st))

            def fwd_train():
                _lib.check(lib.m2t_transblock_forward_train(_lib.ptr(flat), _lib.ptr(x), _lib.ptr(y), B, N, code, _lib.ptr(ws_t), st))

            def bwd():
                _lib.check(lib.m2t_transblock_backward(_lib.ptr(flat), _lib.ptr(gy), _lib.ptr(gx), _lib.ptr(gp), B, N, code, _lib.ptr(ws_t), st))

            def bwd_data():
                _lib.check(lib.m2t_transblock_backward(_lib.ptr(flat), _lib.ptr(gy), _lib.ptr(gx), None, B, N, code, _lib.ptr(ws_t), st))

            def eager():
                torch.autograd.grad(eager_block(xe, pe), [xe] + list(pe.values()), gye)

            arms = {"infer": infer, "fwd_train": fwd_train, "bwd": bwd, "bwd_data": bwd_data, "eager": eager}
            for k in ARMS:                                   # fwd_train comes before the backward arms: they read its workspace
                timed(arms[k], max(1, args.warmup))
            rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
            grad_rel = max(rel(gx, want[0]), rel(gp, want_flat))
            ms = {k: [] for k in ARMS}
            for _ in range(args.repeats):
                for k in ARMS:
                    ms[k].append(timed(arms[k], args.calls))
            cases.append(case_result(N, dtype, ms, ws_t.numel(), grad_rel))
            del ws_i, ws_t, pe, xe, gye
    out = {"workload": "TransBlock(dim=64, 8 heads, chunks of N // 16 tokens): inference forward, training forward, backward, "
                       "backward without parameter gradients, eager torch forward + backward",
           "batch": B, "repeats": args.repeats, "calls": args.calls, "cases": cases}
    assert tuple(out) == RESULT_KEYS
    print(json.dumps(out))


if __name__ == "__main__":
    main()
