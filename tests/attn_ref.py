"""Operator-level gate of the halo window attention: fp64 reference, bf16 error budget, per-pixel-class comparator.

Plain helper module (CPU only, no pytest hooks), shared by tests/test_attn_reference_cpu.py and tests/test_gpu_attn_ops.py.

REFERENCE.  ``reference()`` is oracle.m2trans_oracle.window_attention_core in float64 under autograd, on exactly the values the
kernel sees (``make_inputs`` rounds q | k | v and dO to the storage type first; the rel-pos tables stay fp32: the kernels read
them as fp32).

BUDGET.  ``explicit()`` restates the forward AND the backward per window, without autograd:
    K^ = k + rel            S = q K^T C^-1/2        P = softmax(S)          out = P V
    dP = dO V^T             delta = sum_key P dP    dS = P (dP - delta) C^-1/2
    dq = dS K^              dK^ = dS^T q            dV = P^T dO
    dk | dv = overlap-add of the windows' dK^ | dV rows over the (<= 4) windows whose 10x10 neighbourhood holds the pixel
    drel_h[i] = sum_windows sum_j dK^[10 i + j][: C/2]        drel_w[j] = sum_windows sum_i dK^[10 i + j][C/2 :]
(phantom keys -- the zero padding of k | v outside the image -- carry K^ = rel alone, take softmax mass, contribute to drel
and lose their dk | dv).  With ``points`` empty and float64 it equals the reference to rounding (tests/test_attn_reference_cpu.py:
<= 1e-12).  With the points of a kernel switched on, a value -> bf16 -> value round trip is applied wherever that kernel holds a
bf16 value; the BUDGET of a tensor (or of a pixel class of it) is the own-norm error of that emulation against the reference.
Only this arithmetic feeds the budget: nothing from a HIP run does.  C^-1/2 is a power of two for C = 16, 64, 256, so whether
a kernel scales q (k_attn_c16.hip, exactly, when it stages q), the fp32 scores or dS (k_attn_res.hip) moves no rounding.

ROUNDING POINTS, per kernel (all MFMA accumulation, the softmax, delta and every sum are fp32 and are not rounding points):
  k_attn_c16.hip  window_attn_fwd_c16_kernel          "khat"  K^ = bf16(k + rel_fp32), MFMA operand (registers)
    (bf16 C = 16)                                     "p"     P = bf16(e / sum), operand of O^T = V^T P^T
                                                      "out"   the stored output
                  window_attn_bwd_c16_kernel          "khat"  K^ in registers and in LDS (Kh)
                                                      "p"     P in LDS (Pq), operand of dV; delta and dS use the fp32 P
                                                      "ds"    dS' = bf16(P (dP - delta)) in LDS (Dq) and registers: operand of dq AND dK^
                                                      "dq"    the stored dq (the factor C^-1/2 is applied to the fp32 accumulator)
                                                      "win"   dK^ | dV rows: own pixels -> gqkv, ring keys -> the window scratch `win`
                                                      --      drel: fp32 dK^ accumulators summed in fp32 (NO rounding)
  k_attn_res.hip  window_attn_fwd_res_kernel          "khat", "p", "out" as above (K^ and P in LDS)
    (bf16 C = 64, 256)
                  window_attn_bwd_res_kernel          "khat", "p", "ds", "dq", "win" as above (Kh, Pq, Dq, QOUT / KOUT / VOUT in LDS)
                                                      "relsum" the row / column sums of the ROUNDED dS are stored to LDS as bf16 (Dq columns
                                                              128.. / 144..) and drel = q^T sums comes out of the dK^ MFMA chain
  k_attn.hip      halo_gather_kernel<bf16_t>          "halo"  border pixels: bf16(own row + ring rows of the neighbouring windows), fp32 adds of
    (every bf16 C)                                            bf16 values
                  rel_reduce1 / rel_reduce2           --      fp32 sums over the windows
                  window_attn_fwd_kernel<float> / window_attn_bwd_kernel<float> (fp32, every C): no bf16 value anywhere.
q, k, v and dO are bf16 operands too, but they are the kernel's INPUTS: rounded once by make_inputs for both sides.

COMPARATOR.  ``errors()``: own-norm L2 error || got - ref || / || ref || of out, dq, dk, dv, drel_h, drel_w over the whole tensor
and restricted to pixel classes (``pixel_classes``), because some faults live on a few pixels only:
  out, dq   pixels of image-corner / image-edge / interior WINDOWS (the number of phantom keys differs);
  dk, dv    image-border pixels, and the other pixels by the number of key windows that hold them: 1, 2 (rows / columns 0 or 7
            mod 8 next to another window) or 4 (both).
GATES.  bf16 (``gate_bf16``): every entry <= MARGIN x its budget, MARGIN = 3 as in tests/test_gpu_baseline_configs.py ("no further
from fp64 than 3x the oracle itself").  fp32 (``gate_fp32``): every entry <= 2e-5 (out) / 5e-5 (gradients).  The max-norm metric
of tests/gpu_util.rel at the tolerances of tests/test_gpu_ops.py is kept in both.  The margin is not a knob: a correct kernel that
exceeds it has a rounding point that is missing above.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import m2trans_oracle as O

BLOCK, KWIN, HALO = 8, 10, 1
MARGIN = 3.0
TENSORS = ("out", "dq", "dk", "dv", "drel_h", "drel_w")
FP32_TOL = {"out": 2e-5, "dq": 5e-5, "dk": 5e-5, "dv": 5e-5, "drel_h": 5e-5, "drel_w": 5e-5}
REL_TOL = {"fp32": {"fwd": 2e-5, "bwd": 5e-5}, "bf16": {"fwd": 2e-2, "bwd": 4e-2}}      # tests/test_gpu_ops.py
CONDITIONING_CAP = 1e-2

POINTS_C16 = frozenset({"khat", "p", "out", "ds", "dq", "win", "halo"})
POINTS_RES = POINTS_C16 | {"relsum"}
POINTS_ORACLE_EMU = frozenset({"khat", "p"})      # what O.window_attention_core(emu=_Emu()) rounds


def kernel_points(C: int) -> frozenset:
    """The bf16 rounding points of the kernels m2t_window_attention_fwd / _bwd dispatch to at this C."""
    return POINTS_C16 if C == 16 else POINTS_RES


# (B, h, w): see the geometry table of tests/test_gpu_attn_ops.py
GEOMETRIES = ((1, 8, 8), (1, 8, 16), (1, 16, 8), (3, 8, 24), (1, 24, 24), (2, 16, 24), (1, 40, 56), (2, 32, 72))
REGIMES = ("randn", "kzero", "grid")
CHANNELS = (16, 64, 256)
SEEDS = (3, 5)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def make_inputs(C: int, B: int, h: int, w: int, regime: str, seed: int, dtype: str) -> dict:
    """float32 NCHW q | k | v | gout (already rounded to the storage type `dtype`) and the fp32 rel-pos tables [10][C/2].

    randn  today's tests: randn * 0.7, rel * 0.8, gout ~ N(0, 1).
    kzero  k = 0: the logits are q . rel alone, real and phantom keys compete on equal terms.
    grid   every value a multiple of 2^-3 with |k + rel| < 32, so that k + rel and the bf16 input rounding are exact and only the
           P / dS / output roundings remain.  The last sqrt(C) / 4 channels carry a constant K^ (k = 0, rel_w = 8 in every column) and
           q = +-50 (one sign per query): every raw logit of a query is shifted by +-100 -- beyond the +-88.7 where exp() leaves
           fp32 without the max subtraction -- while the softmax itself is set by the other channels (|q| <= 2: peaked, top
           key below 0.9 of the mass).  The constant K^ is kept small and q large because dq of those channels is K^ sum_key dS
           = 0 exactly: whatever the roundings of dS leave there is pure noise, in proportion to K^.  The shift sits in the
           LAST channels so that an fp32 kernel that accumulates the channels in order does not carry it through every
           partial sum."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + 13 * h + w + B)
    half = C // 2
    if regime in ("randn", "kzero"):
        qkv = torch.randn(B, 3 * C, h, w, generator=g) * 0.7
        rel_h = torch.randn(KWIN, half, generator=g) * 0.8
        rel_w = torch.randn(KWIN, half, generator=g) * 0.8
        gout = torch.randn(B, C, h, w, generator=g)
        if regime == "kzero":
            qkv[:, C:2 * C] = 0.0
    elif regime == "grid":
        def grid(*shape, lim):
            return torch.randint(-lim, lim + 1, shape, generator=g).float() / 8.0
        qkv = torch.cat((grid(B, C, h, w, lim=16), grid(B, C, h, w, lim=12), grid(B, C, h, w, lim=16)), dim=1)
        rel_h, rel_w = grid(KWIN, half, lim=8), grid(KWIN, half, lim=8)
        gout = grid(B, C, h, w, lim=16)
        m = max(1, int(round(math.sqrt(C))) // 4)
        sign = torch.randint(0, 2, (B, 1, h, w), generator=g).float() * 2.0 - 1.0
        qkv[:, C - m:C] = 50.0 * sign
        qkv[:, 2 * C - m:2 * C] = 0.0
        rel_w[:, half - m:] = 8.0
    else:
        raise ValueError(regime)
    if dtype == "bf16":
        qkv, gout = bf16_round(qkv), bf16_round(gout)
    q, k, v = (t.contiguous() for t in torch.chunk(qkv, 3, dim=1))
    return {"q": q, "k": k, "v": v, "rel_h": rel_h, "rel_w": rel_w, "gout": gout}


def reference(inp: dict, dtype=torch.float64, emu=None) -> dict:
    """O.window_attention_core + autograd in `dtype` (float64: THE reference; float32: the oracle's own error)."""
    half = inp["rel_h"].shape[1]
    q, k, v = (inp[n].to(dtype).clone().requires_grad_(True) for n in ("q", "k", "v"))
    rh = inp["rel_h"].to(dtype).reshape(1, KWIN, 1, half).clone().requires_grad_(True)
    rw = inp["rel_w"].to(dtype).reshape(1, 1, KWIN, half).clone().requires_grad_(True)
    out = O.window_attention_core(q, k, v, rh, rw, emu)
    out.backward(inp["gout"].to(dtype))
    return {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad,
            "drel_h": rh.grad.reshape(KWIN, half), "drel_w": rw.grad.reshape(KWIN, half)}


def to_windows(x: torch.Tensor) -> torch.Tensor:
    """[B,C,h,w] -> the 8x8 query windows [B*nh*nw, 64, C]."""
    B, C, h, w = x.shape
    nh, nw = h // BLOCK, w // BLOCK
    return x.view(B, C, nh, BLOCK, nw, BLOCK).permute(0, 2, 4, 3, 5, 1).reshape(B * nh * nw, BLOCK * BLOCK, C)


def from_windows(xw: torch.Tensor, B: int, h: int, w: int) -> torch.Tensor:
    nh, nw = h // BLOCK, w // BLOCK
    C = xw.shape[-1]
    return xw.view(B, nh, nw, BLOCK, BLOCK, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, h, w)


def to_key_windows(x: torch.Tensor) -> torch.Tensor:
    """[B,C,h,w] -> the 10x10 key neighbourhoods of the zero-padded plane [B*nh*nw, 100, C]."""
    B, C, h, w = x.shape
    L = (h // BLOCK) * (w // BLOCK)
    u = F.unfold(x, KWIN, padding=HALO, stride=BLOCK)                    # [B, C*100, L]
    return u.view(B, C, KWIN * KWIN, L).permute(0, 3, 2, 1).reshape(B * L, KWIN * KWIN, C)


def overlap_add(xw: torch.Tensor, B: int, h: int, w: int) -> torch.Tensor:
    """adjoint of to_key_windows: [B*nh*nw, 100, C] -> [B,C,h,w]; rows of phantom keys are dropped."""
    L = (h // BLOCK) * (w // BLOCK)
    C = xw.shape[-1]
    u = xw.view(B, L, KWIN * KWIN, C).permute(0, 3, 2, 1).reshape(B, C * KWIN * KWIN, L)
    return F.fold(u, (h, w), KWIN, padding=HALO, stride=BLOCK)


def rel_bias(rel_h: torch.Tensor, rel_w: torch.Tensor) -> torch.Tensor:
    """[100, C]: key (kr, kc) gets rel_h[kr] on the first C/2 channels and rel_w[kc] on the last."""
    half = rel_h.shape[1]
    return torch.cat((rel_h.view(KWIN, 1, half).expand(KWIN, KWIN, half), rel_w.view(1, KWIN, half).expand(KWIN, KWIN, half)),
                     dim=-1).reshape(KWIN * KWIN, 2 * half)


def explicit(inp: dict, points=frozenset(), dtype=torch.float64) -> dict:
    """The per-window forward and backward formulas of the module docstring with a bf16 round trip at each point in `points`."""
    unknown = set(points) - POINTS_RES
    if unknown:
        raise ValueError(f"unknown rounding points {sorted(unknown)}")

    def r(x, name):
        return bf16_round(x) if name in points else x

    q, k, v, gout = (inp[n].to(dtype) for n in ("q", "k", "v", "gout"))
    rel_h, rel_w = inp["rel_h"].to(dtype), inp["rel_w"].to(dtype)
    B, C, h, w = q.shape
    half = C // 2
    scale = float(C) ** -0.5
    qw, gw = to_windows(q), to_windows(gout)                             # [N, 64, C]
    kw, vw = to_key_windows(k), to_key_windows(v)                        # [N, 100, C]
    N = qw.shape[0]
    kh = r(kw + rel_bias(rel_h, rel_w), "khat")
    S = torch.bmm(qw, kh.transpose(1, 2)) * scale
    P = torch.softmax(S, dim=-1)
    Pb = r(P, "p")
    out = r(torch.bmm(Pb, vw), "out")
    dP = torch.bmm(gw, vw.transpose(1, 2))
    delta = (P * dP).sum(-1, keepdim=True)
    dS = r(P * (dP - delta) * scale, "ds")
    dq = r(torch.bmm(dS, kh), "dq")
    dkh = torch.bmm(dS.transpose(1, 2), qw)                              # [N, 100, C]
    dvw = torch.bmm(Pb.transpose(1, 2), gw)
    if "relsum" in points:
        d4 = dS.view(N, BLOCK * BLOCK, KWIN, KWIN)
        rows, cols = r(d4.sum(3), "relsum"), r(d4.sum(2), "relsum")      # [N, 64, 10]
        drel_h = torch.einsum("nqi,nqc->ic", rows, qw[..., :half])
        drel_w = torch.einsum("nqj,nqc->jc", cols, qw[..., half:])
    else:
        d4 = dkh.view(N, KWIN, KWIN, C)
        drel_h = d4[..., :half].sum((0, 2))
        drel_w = d4[..., half:].sum((0, 1))
    dkh, dvw = r(dkh, "win"), r(dvw, "win")
    dk = r(overlap_add(dkh, B, h, w), "halo")
    dv = r(overlap_add(dvw, B, h, w), "halo")
    # dk_win | dv_win: the windows' dK^ | dV rows [N, 100, C] as the kernel holds them BEFORE the overlap-add (tests/bwd_stage_ref.py:
    # the fused projection data gradient multiplies these rows by Wqkv per window); not in TENSORS, so errors() leaves them alone
    return {"out": from_windows(out, B, h, w), "dq": from_windows(dq, B, h, w), "dk": dk, "dv": dv, "drel_h": drel_h, "drel_w": drel_w,
            "dk_win": dkh, "dv_win": dvw}


# ------------------------------------------------------------------------------------------------ comparator
def pixel_classes(h: int, w: int) -> dict:
    """{'q': {class: bool [h, w]}, 'kv': {class: bool [h, w]}}; empty classes are left out."""
    nh, nw = h // BLOCK, w // BLOCK
    y, x = torch.arange(h).view(h, 1).expand(h, w), torch.arange(w).view(1, w).expand(h, w)
    wy, wx, py, px = y // BLOCK, x // BLOCK, y % BLOCK, x % BLOCK
    by, bx = (wy == 0) | (wy == nh - 1), (wx == 0) | (wx == nw - 1)
    qcls = {"win_corner": by & bx, "win_edge": by ^ bx, "win_interior": ~by & ~bx}
    cy = 1 + (((py == 0) & (wy > 0)) | ((py == BLOCK - 1) & (wy < nh - 1))).long()
    cx = 1 + (((px == 0) & (wx > 0)) | ((px == BLOCK - 1) & (wx < nw - 1))).long()
    border = (y == 0) | (y == h - 1) | (x == 0) | (x == w - 1)
    cover = cy * cx
    kcls = {"img_border": border}
    for n in (1, 2, 4):
        kcls[f"cover{n}"] = (cover == n) & ~border
    return {"q": {n: m for n, m in qcls.items() if bool(m.any())}, "kv": {n: m for n, m in kcls.items() if bool(m.any())}}


def own_norm_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def max_norm_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """tests/gpu_util.rel: largest error over the tensor's largest value."""
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def errors(got: dict, ref: dict) -> dict:
    """{(tensor, class): own-norm L2 error}; class 'all' is the whole tensor.  `got` may hold a subset of TENSORS."""
    e = {}
    h, w = ref["out"].shape[-2:]
    cls = pixel_classes(h, w)
    for t in TENSORS:
        if t not in got:
            continue
        e[(t, "all")] = own_norm_err(got[t], ref[t])
        masks = cls["q"] if t in ("out", "dq") else (cls["kv"] if t in ("dk", "dv") else {})
        for name, m in masks.items():
            e[(t, name)] = own_norm_err(got[t][..., m], ref[t][..., m])
    return e


def budget(inp: dict, ref: dict, C: int) -> dict:
    """bf16 error budget: the emulation with the rounding points of the kernels at this C against the fp64 reference."""
    return errors(explicit(inp, kernel_points(C)), ref)


def _max_norm_failures(got, ref, dt):
    bad = []
    for t in TENSORS:
        if t in got:
            m, tol = max_norm_err(got[t], ref[t]), REL_TOL[dt]["fwd" if t == "out" else "bwd"]
            if not m < tol:
                bad.append(f"{t}: max-norm error {m:.3e} >= {tol:g}")
    return bad


def gate_bf16(got: dict, ref: dict, bud: dict):
    """-> (failures, {(tensor, class): (error, budget, error / budget)})."""
    err = errors(got, ref)
    table = {k: (e, bud[k], e / bud[k] if bud[k] > 0 else (0.0 if e == 0 else math.inf)) for k, e in err.items()}
    bad = [f"{t}[{c}]: error {e:.3e} > {MARGIN:g} x budget {b:.3e} (ratio {q:.2f})" for (t, c), (e, b, q) in table.items()
           if not e <= MARGIN * b]
    return bad + _max_norm_failures(got, ref, "bf16"), table


def gate_fp32(got: dict, ref: dict, oracle32: dict | None = None):
    """-> (failures, {(tensor, class): (error, tolerance, error / float32 oracle's own error)})."""
    err = errors(got, ref)
    o32 = errors({t: oracle32[t] for t in got}, ref) if oracle32 is not None else {}
    table = {k: (e, FP32_TOL[k[0]], e / o32[k] if o32.get(k, 0) > 0 else math.nan) for k, e in err.items()}
    bad = [f"{t}[{c}]: error {e:.3e} > {tol:g}" for (t, c), (e, tol, _) in table.items() if not e <= tol]
    return bad + _max_norm_failures(got, ref, "fp32"), table


def format_table(table: dict, third: str = "ratio") -> str:
    return "\n".join(f"    {t:7s} {c:13s} err {e:.3e}  ref {b:.3e}  {third} {q:6.2f}" for (t, c), (e, b, q) in table.items())
