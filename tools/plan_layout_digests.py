"""Digests of everything a plan's passes leave behind, for comparing two builds of libm2t.so whose workspace layouts must be equal
(the parent's and this tree's, when the host layer's layout code changes): identical offsets mean identical bytes.

    python tools/plan_layout_digests.py --lib /path/to/libm2t.so --out a.json       # one process per library
    python tools/plan_layout_digests.py --compare a.json b.json [--table out.txt]   # exit status 1 unless every digest is equal

Geometry: B = 2, LR 3 x 40 x 56 (pads to 64 x 64), 3 blocks; bf16 and fp32 at x2, x3 and x4.  Modes: a training step (forward,
deferred L1, backward); the same with health = 2; an inference forward; an inference forward with local_norm = 8.  Every workspace
is zeroed and initialised again before the pass, so a region a pass only partly writes has the same bytes in both processes.
Recorded per mode: the sha256 of sr, of the flat gradients, of the health record, and of every named workspace region that is
present (the bytes from its offset to the next region's, so the alignment gaps are covered).
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H0, W0, NB = 2, 40, 56, 3
MODES = ("train", "train_health2", "infer", "infer_local_norm8")
EXTRA = ("xn", "lnsum", "norm_id", "health", "health_part", "health_descs", "health_work")


def run(lib_path):
    import torch
    from m2trans_amd import _lib
    _lib.LIB_PATH = lib_path
    lib = _lib.load()
    from m2trans_amd.M2Trans_network import Plan
    from oracle import m2trans_oracle as O
    from tests.gpu_util import build_model
    from tests.test_lean_plan_cpu import all_names
    sha = lambda t: hashlib.sha256(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
    out = {}
    for dtype in ("bf16", "fp32"):
        for scale in (2, 3, 4):
            model, _ = build_model(scale, NB, dtype)
            dev = model.flat_params.device
            code = _lib.F32 if dtype == "fp32" else _lib.BF16
            x = O.closed_form_image(B, 3, H0, W0).cuda()
            hr = O.closed_form_image(B, 3, H0 * scale, W0 * scale, phase=0.7).cuda()
            for mode in MODES:
                train = mode.startswith("train")
                plan = Plan(B, H0, W0, scale, NB, code, dev, inference=not train, local_norm=8 if mode.endswith("norm8") else 0,
                            options={"health": 2} if mode.endswith("health2") else None)
                st, ws = _lib.stream_ptr(), _lib.ptr(plan.workspace)
                plan.workspace.zero_()
                _lib.check(lib.m2t_plan_init_workspace(plan.handle, ws, st), "m2t_plan_init_workspace")
                rec = {}
                rec["sr"] = sha(model._run_forward(plan, x, keep=train))
                if train:
                    loss = torch.zeros(1, dtype=torch.float32, device=dev)
                    grads = torch.zeros_like(model.flat_params)
                    _lib.check(lib.m2t_l1_loss_deferred(plan.handle, _lib.ptr(hr), 1.0, float(hr.numel()), float(model.rgb_range),
                                                        _lib.ptr(loss), ws, st), "m2t_l1_loss_deferred")
                    _lib.check(lib.m2t_backward(plan.handle, _lib.ptr(model.flat_params), _lib.ptr(x), _lib.ptr(grads), ws, st), "m2t_backward")
                    rec["grads"], rec["loss"] = sha(grads), sha(loss)
                torch.cuda.synchronize()
                total = plan.query("workspace_bytes")
                offs = {n: int(lib.m2t_plan_query(plan.handle, ("ws:" + n).encode())) for n in all_names(NB, 4) + list(EXTRA)}      # (-1: absent)
                starts = sorted({o for o in offs.values() if o >= 0}) + [total]
                for n, o in offs.items():
                    if o >= 0:
                        rec["ws:" + n] = sha(plan.workspace[o:starts[starts.index(o) + 1]])
                rec["workspace_bytes"] = str(total)
                out[f"{dtype} x{scale} {mode}"] = rec
                del plan
    return out


def compare(a_path, b_path, table):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    lines = [f"# {'plan and mode':32s} {'digests':>7s} {'equal':>5s}  sr                grads             health            all regions"]
    bad = sorted(set(a) ^ set(b))
    for k in a:
        if k not in b:
            continue
        ra, rb = a[k], b[k]
        same = sum(1 for n in ra if rb.get(n) == ra[n])
        if same != len(ra) or len(ra) != len(rb):
            bad += [f"{k}: {n}" for n in sorted(set(ra) | set(rb)) if ra.get(n) != rb.get(n)]
        every = hashlib.sha256("".join(f"{n}={v};" for n, v in sorted(ra.items())).encode()).hexdigest()
        cell = lambda n: ra.get(n, "-")[:16]
        lines.append(f"{k:34s} {len(ra):7d} {same:5d}  {cell('sr'):16s}  {cell('grads'):16s}  {cell('ws:health'):16s}  {every[:16]}")
    lines.append(f"# {'every digest of the two libraries is equal' if not bad else 'DIFFERENT: ' + '; '.join(bad[:20])}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if table:
        open(table, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--table")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.table))
    result = run(os.path.abspath(args.lib))
    json.dump(result, open(args.out, "w"), indent=0)
    print(f"{len(result)} modes, {sum(len(r) for r in result.values())} digests -> {args.out}")
