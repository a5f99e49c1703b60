"""ms / step of the BASELINE configs[2] training step (x4, 128^2 LR, batch 32, bf16, L1 + lambda_clip 0.01 SemanticLoss, N_patches 3)
with the default SemanticLoss (a constant term, no gradient) and with SemanticLoss(differentiable=True) (its gradient reaches the
model), in one process on one device: HIP events around `--steps` warm steps of each.  Prints one JSON line.

    python tools/semantic_grad_timing.py [--steps 10] [--warmup 3] [--dtype bf16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def swin_state(dtype_code, B, device):
    """The random-init tower bench.py uses for configs[2]."""
    from m2trans_amd.losses import SwinEncoder
    e = SwinEncoder(2, dtype_code, device)
    g = torch.Generator().manual_seed(33)
    state = {n: (torch.randn(k, generator=g) * (0.02 if "weight" in n and "norm" not in n else 0.0)
                 + (1.0 if n.endswith("norm.weight") or ("layernorm" in n and n.endswith("weight")) else 0.0))
             for n, (o, k) in e.slots.items()}
    del e
    return state


def time_mode(differentiable, args, device, state):
    from m2trans_amd.M2Trans_network import create_model
    from m2trans_amd.losses import SemanticLoss
    from m2trans_amd.train_step import TrainStep
    import types
    B = args.batch
    margs = types.SimpleNamespace(n_feats=64, scale=4, rgb_range=1.0, n_blocks=8, colors=3, compute_dtype=args.dtype)
    model = create_model(margs).to(device)
    sem = SemanticLoss(criterion="l1", N_patches=3, device=device, compute_dtype=args.dtype, max_batch=B, synthetic_text=True,
                       differentiable=differentiable)
    sem.load_image_encoder(state)
    caps = [f"synthetic ultrasound caption {i}" for i in range(B)]
    ts = TrainStep(model, lr=1e-4, world_size=1, semantic_loss=sem, lambda_clip=0.01)
    g = torch.Generator(device=device).manual_seed(33)
    batches = [(torch.rand(B, 3, 128, 128, generator=g, device=device), torch.rand(B, 3, 512, 512, generator=g, device=device))
               for _ in range(2)]
    for s in range(args.warmup):
        ts.step(*batches[s % 2], caps)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for s in range(args.steps):
        loss = ts.step(*batches[s % 2], caps)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / args.steps
    finite = bool(torch.isfinite(loss).all()) and bool(torch.isfinite(ts.grads).all())
    del ts, model, sem
    torch.cuda.empty_cache()
    return ms, finite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    from m2trans_amd import _lib
    _lib.load()
    device = torch.device("cuda", 0)
    state = swin_state(_lib.F32 if args.dtype == "fp32" else _lib.BF16, args.batch, device)
    base, ok0 = time_mode(False, args, device, state)
    diff, ok1 = time_mode(True, args, device, state)
    print(json.dumps({"workload": "configs[2] step, SemanticLoss default vs differentiable", "dtype": args.dtype, "batch": args.batch,
                      "steps": args.steps, "ms_per_step_default": round(base, 3), "ms_per_step_differentiable": round(diff, 3),
                      "ratio": round(diff / base, 3), "budget_ratio": 1.4, "finite": ok0 and ok1}))


if __name__ == "__main__":
    main()
