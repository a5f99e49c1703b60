"""ms per forward / forward + backward of the configs[1] geometry (x4, 8 blocks, batch 16, 128^2 LR) through the autograd node, with
and without the input gradient and with frozen stages, in one process on one device: HIP events around `--steps` warm iterations of
each mode.  Prints one JSON line.

    (a) forward alone (training forward: activations kept, no backward)
    (b) forward + backward, every weight trainable (today's path, m2t_backward)
    (c) (b) with lr.requires_grad (m2t_backward_ex: every stage + the input gradient)
    (d) frozen model, lr.grad only (no parameter-gradient work at all)
    (e) only the tail trainable, lr without gradient

    python tools/input_grad_timing.py [--steps 20] [--warmup 5] [--dtype bf16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def time_mode(model, lr, g_sr, need_x, backward, args):
    def it():
        x = lr.detach().requires_grad_(need_x)
        sr = model(x)
        if backward:
            sr.backward(g_sr)
    for _ in range(args.warmup):
        it()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(args.steps):
        it()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / args.steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    from m2trans_amd.M2Trans_network import create_model
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=8, colors=3, compute_dtype=args.dtype)
    model = create_model(margs).to(device)
    g = torch.Generator(device=device).manual_seed(33)
    lr = torch.rand(args.batch, 3, 128, 128, generator=g, device=device)
    g_sr = torch.randn(args.batch, 3, 512, 512, generator=g, device=device) * 1e-3
    ms = {}
    ms["a_forward"] = time_mode(model, lr, g_sr, False, False, args)
    ms["b_fwd_bwd"] = time_mode(model, lr, g_sr, False, True, args)
    ms["c_fwd_bwd_input_grad"] = time_mode(model, lr, g_sr, True, True, args)
    model.requires_grad_(False)
    ms["d_frozen_input_grad"] = time_mode(model, lr, g_sr, True, True, args)
    model.tail.requires_grad_(True)
    ms["e_tail_only"] = time_mode(model, lr, g_sr, False, True, args)
    bwd = {k: ms[k] - ms["a_forward"] for k in ms if k != "a_forward"}
    print(json.dumps({"workload": "configs[1] geometry forward / backward through the autograd node", "dtype": args.dtype,
                      "batch": args.batch, "steps": args.steps, **{k: round(v, 4) for k, v in ms.items()},
                      "c_minus_b_us": round(1e3 * (ms["c_fwd_bwd_input_grad"] - ms["b_fwd_bwd"]), 1),
                      "bwd_ratio_d_over_b": round(bwd["d_frozen_input_grad"] / bwd["b_fwd_bwd"], 3),
                      "bwd_ratio_e_over_b": round(bwd["e_tail_only"] / bwd["b_fwd_bwd"], 3),
                      "budget": {"c_minus_b_us": 15, "bwd_ratio_d_over_b": 0.8, "bwd_ratio_e_over_b": 0.3}}))


if __name__ == "__main__":
    main()
