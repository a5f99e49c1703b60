"""Teacher-forced stage gate of the backward pass: fp64 reference per stage, bf16 error budget, per-pixel-class comparator.

Plain helper module (CPU only, no pytest hooks), shared by tests/test_bwd_stage_reference_cpu.py and tests/test_gpu_bwd_stages.py;
the mirror image of the forward stage gate (tests/test_gpu_baseline_configs.py check_vs_oracle) and the model-level continuation of
tests/attn_ref.py.

TAPS.  Gradient tensors that a synchronised m2t_backward_ex of a model with n_blocks <= 2 leaves in the workspace (read from the body
loop and the head part of backward_impl in csrc/m2t_api.hip; tests/gpu_util.hip_backward_trace reads them back), under these names:
  gpre          fp32 seed [B,3,Hsp,Wsp] (padded size, zero outside the crop and under a live clamp): m2t_set_output_grad
  g_t1pre       x4 only: gradient of the first expansion's pre-activation [B,64,2H,2W]
  gT            gradient of X[n_blocks], the tail's input (written by the tail backward alone)
  gB            two blocks: gradient of X1 (block 1's InstanceNorm backward, gnext[1])
  b<b>.gqkv<i>  dq | dK | dV of branch i = 1..4 of block b, buffer set b & 1 (workspace names gqkv<i-1> / gqkv<i-1>b); the overlap-add of
                dK | dV is complete after halo_gather (side stream, fused projection), c16_dgrad_prep or window_attn_bwd's own gather
  gn            block 0: gradient of the InstanceNorm output, four planes; projection data gradient + ring overlap-add + branch_prep_bwd
                of every branch -- the identity path does not pass through it
  gres          the workspace region gxc after block 0's launch_instnorm_bwd: g(res) = g(X0) + g(Y), the head's cotangent
  lr.grad       the input gradient m2t_backward_ex returns (fp32)
LEFT OUT, because a later launch of the same pass overwrites them (csrc/m2t_api.hip, backward_impl):
  gxc as the 3x3 conv's data gradient   branch_prep_bwd / c16_dgrad_prep / the PB phase of window_attn_bwd_res_kernel add the branch chain into
                                        planes 0..2 ("store_ch(gxc + (k - 1) ...)"), then launch_instnorm_bwd of block 0 writes g(res) over it
  gn, gxc of block 1 (two blocks)       block 0's launches write the same regions
  gd, gdwin (gd2, gdwin2)               every branch writes them (launch_window_attn_bwd_resident / launch_gemm_nt); branches 4 and 2 share gd
  win<i>                                complete, but only the ring half of what gqkv already holds after the overlap-add
  g_t2pre                               bf16 default: lives in LDS only (k_tail_bwd.hip); the plain path stores it, no schedule-independent tap
  g_t1pre of x2 / x3                    bf16 default: g(t) lives in LDS only (k_tail_bwd_stream.hip)
  gA                                    n_blocks >= 3 only

REFERENCE.  ``build_graph`` runs oracle.m2trans_oracle.forward in float64 under autograd -- bf16 mode: emulate_bf16=True with
force=<hip_forward_trace>, so the gradient flows along the HIP run's own trajectory; fp32 mode: the plain restatement.  ``stage_refs``
gives each tap's reference as the VJP from the nearest intact upstream tap, with the run's OWN value of that tap as cotangent:
  gpre -> g_t1pre -> gT (x4) or gpre -> gT (x2 / x3);  gy -> b.gqkv_i, gy -> gn (block 0), gT -> gB (block 1 of two), with gy = gT for the
  last block and gB for block 0 of two;  (gn, gy, gT) -> gres = InstanceNorm VJP(gn) + gy + gT as launch_instnorm_bwd adds them;
  gres -> lr.grad: adjoint of the reflect-padded head conv including the fold of the padded rows and columns.
gpre itself is checked against g(sr) x clamp mask read from the run's srpre (``seed``).  With chain=True each stage takes the previous
stage's REFERENCE as cotangent; from the oracle's own seed that reproduces plain autograd (tests/test_bwd_stage_reference_cpu.py: 1e-12).

BUDGET.  ``emulate`` restates the same chain explicitly (no autograd across stages) with a value -> bf16 -> value round trip wherever the
default bf16 schedule holds a bf16 gradient; the budget of a (tap, class) is the gate's own error of the emulated taps, which play the
device: emulated tap against the VJP of the emulated upstream tap.  Only this arithmetic feeds the budget.  ROUNDING POINTS, per kernel
(every accumulation, the InstanceNorm sums and the Haar butterflies are fp32 and are no rounding points):
  k_tail_bwd.hip  tail_bwd16 / tail_bwd32 kernels (x4)   "geff"   g(sr) gathered into Geff, a bf16 MFMA operand in LDS
                                                          "gt2"    g(t2) = bf16(g(a2) gelu'(t2)) in LDS (g_t2pre of the plain path)
                                                          "gt1"    the stored g_t1pre = bf16((g(u) W3) gelu'(t1))
  k_gemm.hip      gemm_nt (tail.0 data gradient, x4)      "gT"     the stored gT
  k_tail_bwd_stream.hip  tail_bwd_stream_kernel (x2 / x3) "geff", "gt1" (g(t) in LDS), "gT"
  k_conv.hip      conv3x3_c64_bwd_rows_kernel / conv3x3   "gxc"    the stored data gradient of the 3x3 conv
  k_attn_res.hip  window_attn_bwd_res_kernel (C >= 64)    "do"     dO = bf16(DWT^L of the stored g_xc plane), MFMA operand
                                                          the attention's own points: attn_ref.kernel_points(C) (khat, p, ds, dq, win, relsum)
                                                          "gd"     DG: own-window rows of g_d = [dq | dK^ | dV] Wqkv -> gd, ring rows -> gdwin
                                                          "gdsum"  PB (branch 4 inside branch 3's launch): bf16(own rows + ring rows), fp32 adds
                                                          "gn", "gxc"  PB: the stored g_n plane and the re-stored g_xc plane
  k_attn.hip      halo_gather_kernel                      "halo"   (attn_ref) dK | dV of border pixels completed in gqkv
  k_pointwise.hip branch_prep_bwd(_tiled)_kernel          "gdsum"  bf16(g_d + ring rows) (tiled: every row, staged in LDS as bf16)
                                                          "gn"     g_n[k] = bf16((IWT^L g_d + g_xc[k]) / 2);  "gxc"  g_xc[k-1] = bf16(g_xc[k-1] + that)
  k_attn_c16.hip  window_attn_bwd_c16_kernel              "do" and attn_ref.kernel_points(16)
                  c16_dgrad_prep_kernel                   "halo"   dK | dV completed in place in gqkv (bf16)
                                                          "gd"     g_d = bf16(gqkv Wqkv) ("a stored bf16 tensor in the unfused chain");  "gn"
  k_pointwise.hip instnorm_bwd_apply_kernel               "gx"     block 0: bf16(gy + InstanceNorm term), then + gT; the stored result: "gx" again
  k_conv.hip      head_conv_dgrad_kernel                  "chain"  reads the bf16 g(res) and fp32 weights; its OUTPUT is fp32, so the only error of the stage is
                                                                   the accumulation itself: ONE fp32 FMA chain of 9 x 64 = 576 terms per output value, in the order
                                                                   plane q, ky, kx, channel (the folded preimages continue the chain).  Restated in float32 in
                                                                   that order (``_head_adjoint_chain``); a blocked or pairwise sum, as the float32 oracle's, is
                                                                   2-4x more accurate and is no yardstick for it
A fused backward kernel added later puts its storage point where its stage sits in ``_emulate_block`` / ``_emulate_tail``.

COMPARATOR.  ``errors``: own-norm L2 error || got - ref || / || ref || over the whole tap ('all') and per pixel class:
  b.gqkv_i, gn[i] (plane i of gn)   attn_ref.pixel_classes 'kv' (img_border, cover1 / 2 / 4) at the branch's level; a full-resolution pixel of
                                    gn takes the class of its level-L coordinate
  gres, gT, gB                      border (image-border rows and columns; the 3x3 conv is zero-padded) / interior
  gres                              also chan_mean and along_xhat: the [B, 64] per-plane means of gres and of gres * xhat -- the two sums that the
                                    InstanceNorm backward subtracts are below a pixel's bf16 noise, but not below that of a plane's sum
  g_t1pre                           border / interior (the tail conv is reflect-padded)
  lr.grad                           folded (pixels that receive a reflected contribution, from pad_to_multiple or the conv's own ring) /
                                    unfolded, and border / interior
GATES.  bf16 (``gate_bf16``): every entry <= attn_ref.MARGIN (3) x its budget.  Where a budget is exactly zero -- gpre: g(sr) times a 0 / 1
mask, exact in any format -- the FLOOR is the float32 oracle's own error against float64 on the same stage (``stage_refs`` on a float32
graph; for gpre that is zero too: the seed must be bit-exact).  fp32 (``gate_fp32``): <= 1e-4 of own norm, or <= 3 x that float32
oracle error (the rule check_vs_oracle applies to fp32 gradients).  The margin is not a knob: a correct kernel that exceeds it has a
rounding point that is missing above.
"""
from __future__ import annotations

import math
import types

import torch
import torch.nn.functional as F

from oracle import m2trans_oracle as O
from tests import attn_ref as A

BR_C = (16, 64, 256, 256)
BR_L = (0, 1, 2, 2)
FP32_TOL = 1e-4
EPS = 1e-5                      # InstanceNorm (oracle.m2trans_oracle.instance_norm)


def _rnd(x, on=True):
    return A.bf16_round(x) if on else x


# ------------------------------------------------------------------------------------------------ reference graph
def build_graph(x, params, scale, n_blocks, dtype, force=None, ftype=torch.float64, leaf_params=False):
    """One oracle forward under autograd; returns the graph (cap tensors by workspace name, the input leaf, geometry).
    leaf_params: the trainable parameters are leaves too (parameter gradients by autograd)."""
    if n_blocks not in (1, 2):
        raise ValueError("the taps are intact for n_blocks <= 2 only")
    xg = x.detach().to(ftype).clone().requires_grad_(True)
    p = {k: v.detach().to(ftype) for k, v in params.items()}
    if leaf_params:
        p = {k: (v.requires_grad_(True) if k not in O.FROZEN else v) for k, v in p.items()}
    cap = {}
    O.forward(xg, p, scale, n_blocks, return_preclamp=True, cap=cap, emulate_bf16=(dtype == "bf16"), force=force)
    B, _, H0, W0 = x.shape
    H, W = cap["X0"].shape[-2:]
    return types.SimpleNamespace(x=xg, p=p, cap=cap, scale=scale, nb=n_blocks, dtype=dtype, B=B, H0=H0, W0=W0, H=H, W=W, ftype=ftype)


def cotangent(B, Hs, Ws, seed=11):
    """A seeded random smooth cotangent for sr: white noise under a 5x5 box filter (float64)."""
    gen = torch.Generator().manual_seed(seed)
    return F.avg_pool2d(torch.randn(B, 3, Hs + 4, Ws + 4, generator=gen, dtype=torch.float64), 5, stride=1) * 3.0


def seed(g_sr, srpre, rgb_range=1.0):
    """gpre [B,3,Hsp,Wsp]: g(sr) inside the crop where 0 <= srpre <= R (torch.clamp's own mask), zero elsewhere."""
    H0s, W0s = g_sr.shape[-2:]
    out = torch.zeros_like(srpre)
    crop = srpre[..., :H0s, :W0s]
    out[..., :H0s, :W0s] = g_sr.to(srpre.dtype) * ((crop >= 0) & (crop <= rgb_range)).to(srpre.dtype)
    return out


def _vjp(outs, ins, cot):
    return torch.autograd.grad(outs, ins, cot, retain_graph=True)


def stage_refs(g, taps, chain=False):
    """{tap: reference} (g.ftype): the VJP from the nearest upstream tap with `taps`' value of it as cotangent (chain=True: with the
    reference just computed for it; `taps` then needs gpre only)."""
    c, nb = g.cap, g.nb
    refs = {}

    def up(name):
        return (refs[name] if chain and name in refs else taps[name]).to(g.ftype)

    if g.scale == 4:
        (refs["g_t1pre"],) = _vjp(c["srpre"], c["t1pre"], up("gpre"))
        (refs["gT"],) = _vjp(c["t1pre"], c[f"X{nb}"], up("g_t1pre"))
    else:
        (refs["gT"],) = _vjp(c["srpre"], c[f"X{nb}"], up("gpre"))
    for b in range(nb - 1, -1, -1):
        gy = up("gT") if b == nb - 1 else up("gB")
        ins = [c[f"b{b}.qkv{i}"] for i in range(1, 5)] + ([c["b0.xn"]] if b == 0 else [c[f"X{b}"]])
        gr = _vjp(c[f"X{b + 1}"], ins, gy)
        for i in range(4):
            refs[f"b{b}.gqkv{i + 1}"] = gr[i]
        if b == 0:
            refs["gn"] = gr[4]
            # launch_instnorm_bwd of block 0: gres = gy ("+ x" of the feed-forward conv) + InstanceNorm term, then + gT (`res + y`)
            (t,) = _vjp(c["b0.xn"], c["X0"], up("gn"))
            refs["gres"] = t + gy + up("gT")
        else:
            refs["gB"] = gr[4]
    (refs["lr.grad"],) = _vjp(c["X0"], g.x, up("gres"))
    return refs


def autograd_taps(g, g_sr, rgb_range=1.0):
    """Every tap by plain torch.autograd.grad of sum(clamp(sr) * g_sr) through the oracle graph (the consistency test's yardstick)."""
    c, nb = g.cap, g.nb
    H0s, W0s = g.H0 * g.scale, g.W0 * g.scale
    loss = (torch.clamp(c["srpre"][..., :H0s, :W0s], 0.0, rgb_range) * g_sr.to(g.ftype)).sum()
    names = (["g_t1pre"] if g.scale == 4 else []) + ["gT"] + (["gB"] if nb == 2 else []) + ["gn", "gres", "lr.grad"]
    ins = ([c["t1pre"]] if g.scale == 4 else []) + [c[f"X{nb}"]] + ([c["X1"]] if nb == 2 else []) + [c["b0.xn"], c["X0"], g.x]
    for b in range(nb):
        for i in range(1, 5):
            names.append(f"b{b}.gqkv{i}")
            ins.append(c[f"b{b}.qkv{i}"])
    return dict(zip(names, _vjp(loss, ins, None)))


# ------------------------------------------------------------------------------------------------ explicit chain (budget, faults)
FAULTS = ("ring:0", "ring:1", "ring:2", "ring_corner:0", "ring_corner:1", "ring_corner:2", "no_half:3", "haar_sign:1", "in_no_xhat_term",
          "res_once", "conv_border_row", "head_no_fold", "tail_no_reflect")


def _dwt_l(x, L):
    for _ in range(L):
        x = O.dwt(x)
    return x


def _iwt_l(x, L):
    for _ in range(L):
        x = O.iwt(x)
    return x


def _reflect_conv_adjoint(gout, w, in_shape, fold=True):
    """g(input) of O.conv3x3_reflect(input, w); fold=False drops what reached the input through the reflected ring."""
    z = torch.zeros(in_shape, dtype=gout.dtype, requires_grad=True)
    zp = F.pad(z, (1, 1, 1, 1), mode="reflect")
    (gz,) = torch.autograd.grad(F.conv2d(zp, w), z if fold else zp, gout)
    return gz if fold else gz[..., 1:-1, 1:-1]


def _w(g, name, rounded):
    w = g.p[name]
    return _rnd(w) if (rounded and g.dtype == "bf16") else w        # the packed weights are bf16 in bf16 mode (O._rw)


def _emulate_tail(g, gpre, pts, fault):
    c, s = g.cap, g.scale
    fold = fault != "tail_no_reflect"
    last = "tail.6.weight" if s == 4 else "tail.3.weight"
    a_last = c["t2act" if s == 4 else "t1act"]
    ga = _reflect_conv_adjoint(_rnd(gpre, pts), _w(g, last, True), a_last.shape, fold)
    out = {}
    if s == 4:
        gt2 = _rnd(ga * c["t2der"].detach(), pts)
        ga1 = F.conv_transpose2d(F.pixel_unshuffle(gt2, 2), _w(g, "tail.3.weight", True))
        gt1 = out["g_t1pre"] = _rnd(ga1 * c["t1der"].detach(), pts)
        r0 = 2
    else:
        gt1 = _rnd(ga * c["t1der"].detach(), pts)
        r0 = s
    out["gT"] = _rnd(F.conv_transpose2d(F.pixel_unshuffle(gt1, r0), _w(g, "tail.0.weight", True)), pts)
    return out


def _window_dgrad(ex, wq, B, h, w, pts, ring_keep=None):
    """The fused projection data gradient (k_attn_res.hip DG): each window multiplies its own dq | dK^ | dV rows by Wqkv; own pixels ->
    gd, ring keys -> gdwin, overlap-added afterwards.  ring_keep [N] (0 / 1): windows whose ring rows survive (faults)."""
    C = wq.shape[1]
    prod = ex["dk_win"] @ wq[C:2 * C] + ex["dv_win"] @ wq[2 * C:]                           # [N, 100, C]
    N = prod.shape[0]
    p4 = prod.view(N, A.KWIN, A.KWIN, C)
    own = p4[:, 1:9, 1:9].reshape(N, 64, C) + A.to_windows(ex["dq"]) @ wq[:C]
    ring = p4.clone()
    ring[:, 1:9, 1:9] = 0.0
    if ring_keep is not None:
        ring = ring * ring_keep.view(N, 1, 1, 1).to(ring.dtype)
    gd = A.from_windows(_rnd(own, pts), B, h, w)
    return gd + A.overlap_add(_rnd(ring.reshape(N, 100, C), pts), B, h, w)


def _corner_windows(B, h, w):
    nh, nw = h // 8, w // 8
    wy, wx = torch.arange(nh).view(nh, 1).expand(nh, nw), torch.arange(nw).view(1, nw).expand(nh, nw)
    m = ((wy == 0) | (wy == nh - 1)) & ((wx == 0) | (wx == nw - 1))
    return m.reshape(1, nh * nw).expand(B, nh * nw).reshape(-1)


def _emulate_block(g, b, gy, gT, pts, fault, out):
    c, B, H, W = g.cap, g.B, g.H, g.W
    pre = f"body.{b}."
    gxc = _rnd(F.conv_transpose2d(gy, _w(g, pre + "feed_forward.0.weight", True), padding=1), pts)
    if fault == "conv_border_row":
        gxc = gxc.clone()
        gxc[:, :, 0, :] = 0.0
    ch = list(torch.split(gxc, 16, dim=1))
    gn = [None] * 4
    for i in (3, 2, 1, 0):
        C, L = BR_C[i], BR_L[i]
        h, w = H >> L, W >> L
        q, k, v = torch.chunk(c[f"b{b}.qkv{i + 1}"].detach(), 3, dim=1)
        inp = {"q": q, "k": k, "v": v, "rel_h": g.p[pre + f"attn{i + 1}.rel_h"].reshape(A.KWIN, C // 2),
               "rel_w": g.p[pre + f"attn{i + 1}.rel_w"].reshape(A.KWIN, C // 2), "gout": _rnd(_dwt_l(ch[i], L), pts)}
        # (without the kernels' points the bf16 graph still carries the oracle's own forward roundings of K^ and P, straight through)
        ex = A.explicit(inp, A.kernel_points(C) if pts else (A.POINTS_ORACLE_EMU if g.dtype == "bf16" else frozenset()), dtype=g.ftype)
        out[f"b{b}.drel{i + 1}"] = (ex["drel_h"], ex["drel_w"])
        gqkv = out[f"b{b}.gqkv{i + 1}"] = torch.cat((ex["dq"], ex["dk"], ex["dv"]), dim=1)
        wq = _w(g, pre + f"attn{i + 1}.qkv_conv.weight", True).reshape(3 * C, C)
        ring_fault = fault in (f"ring:{i}", f"ring_corner:{i}")
        if C >= 64 or ring_fault:
            keep = None
            if ring_fault:
                keep = ~_corner_windows(B, h, w) if fault.startswith("ring_corner") else torch.zeros(B * (h // 8) * (w // 8), dtype=torch.bool)
            gd = _window_dgrad(ex, wq, B, h, w, pts, keep)
        else:
            gd = F.conv_transpose2d(gqkv, wq.view(3 * C, C, 1, 1))
        gd = _rnd(gd, pts)
        if fault == f"haar_sign:{i}":
            gd = gd.clone()
            gd[:, C // 4:C // 2] *= -1.0               # the second Haar sub-band of the outermost level
        gxin = _iwt_l(gd, L) + ch[i]
        if i == 0:
            gn[0] = _rnd(gxin, pts)
        else:
            half = gxin if fault == f"no_half:{i}" else 0.5 * gxin
            gn[i] = _rnd(half, pts)
            ch[i - 1] = _rnd(ch[i - 1] + half, pts)
    gn = torch.cat(gn, dim=1)
    X = c[f"X{b}"].detach()
    mu = X.mean(dim=(2, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(X.var(dim=(2, 3), unbiased=False, keepdim=True) + EPS)
    xhat = (X - mu) * rstd
    s1 = gn.mean(dim=(2, 3), keepdim=True)
    s2 = (gn * xhat).mean(dim=(2, 3), keepdim=True)
    if fault == "in_no_xhat_term":
        s2 = torch.zeros_like(s2)
    t = gy + rstd * (gn - s1 - xhat * s2)
    if b == 0:
        out["gn"] = gn
        t = _rnd(t, pts) + (0.0 if fault == "res_once" else gT)
    return _rnd(t, pts)


def _head_adjoint_chain(g, gres):
    """head_conv_dgrad_kernel's arithmetic: per value one float32 FMA chain over (plane q, ky, kx, channel) of the zero-padded transposed
    conv on the ring-padded grid, then the fold of the reflected ring and of pad_to_multiple's rows and columns, in float32."""
    B, H, W = g.B, g.H, g.W
    w = g.p["head.weight"].detach().float()
    gp = F.pad(gres.detach().float(), (2, 2, 2, 2))
    acc = torch.zeros(B, 3, H + 2, W + 2, dtype=torch.float32)
    for q in range(4):
        for ky in range(3):
            for kx in range(3):
                for ch in range(16):
                    oc = 16 * q + ch
                    gs = gp[:, oc:oc + 1, 2 - ky:2 - ky + H + 2, 2 - kx:2 - kx + W + 2]
                    # fmaf: the product of two float32 values is exact in float64, the sum is rounded once
                    acc = (acc.double() + w[oc, :, ky, kx].view(1, 3, 1, 1).double() * gs.double()).float()
    z = torch.zeros(B, 3, g.H0, g.W0, dtype=torch.float32, requires_grad=True)
    (out,) = torch.autograd.grad(F.pad(O.pad_to_multiple(z), (1, 1, 1, 1), mode="reflect"), z, acc)
    return out


def emulate(g, gpre, points=True, fault=None):
    """Every tap by the explicit chain from the seed `gpre`; points: the bf16 round trips of the module docstring; fault: one of FAULTS."""
    if fault is not None and fault not in FAULTS:
        raise ValueError(fault)
    gpre = gpre.to(g.ftype)
    out = {"gpre": gpre}
    out.update(_emulate_tail(g, gpre, points, fault))
    gy = out["gT"]
    for b in range(g.nb - 1, -1, -1):
        gy = _emulate_block(g, b, gy, out["gT"], points, fault, out)
        out["gres" if b == 0 else "gB"] = gy
    if fault == "head_no_fold":
        z = torch.zeros(g.B, 3, g.H, g.W, dtype=g.ftype, requires_grad=True)
        (gz,) = torch.autograd.grad(O.conv3x3_reflect(z, g.p["head.weight"]), z, gy)
        out["lr.grad"] = gz[..., :g.H0, :g.W0]
    elif points:
        out["lr.grad"] = _head_adjoint_chain(g, gy)
    else:
        (out["lr.grad"],) = _vjp(g.cap["X0"], g.x, gy)
    return out


# ------------------------------------------------------------------------------------------------ comparator
def _border(h, w):
    y, x = torch.arange(h).view(h, 1).expand(h, w), torch.arange(w).view(1, w).expand(h, w)
    return (y == 0) | (y == h - 1) | (x == 0) | (x == w - 1)


def _folded(g):
    z = torch.zeros(1, 1, g.H0, g.W0, dtype=torch.float64, requires_grad=True)
    (cnt,) = torch.autograd.grad(F.pad(O.pad_to_multiple(z), (1, 1, 1, 1), mode="reflect").sum(), z)
    return cnt[0, 0] > 1.5


def tap_classes(g, tap):
    """[(entry name, channel slice or None, {class: bool [h, w]})] for one tap."""
    def named(d):
        return {n: m for n, m in d.items() if bool(m.any())}
    if tap == "gn":
        res = []
        for i in range(4):
            L = BR_L[i]
            kv = A.pixel_classes(g.H >> L, g.W >> L)["kv"]
            res.append((f"gn[{i + 1}]", slice(16 * i, 16 * i + 16),
                        {n: m.repeat_interleave(1 << L, 0).repeat_interleave(1 << L, 1) for n, m in kv.items()}))
        return res
    if ".gqkv" in tap:
        L = BR_L[int(tap[-1]) - 1]
        return [(tap, None, A.pixel_classes(g.H >> L, g.W >> L)["kv"])]
    if tap in ("gres", "gT", "gB"):
        bd = _border(g.H, g.W)
        return [(tap, None, named({"border": bd, "interior": ~bd}))]
    if tap == "g_t1pre":
        bd = _border(2 * g.H, 2 * g.W)
        return [(tap, None, named({"border": bd, "interior": ~bd}))]
    if tap == "lr.grad":
        bd, fo = _border(g.H0, g.W0), _folded(g)
        return [(tap, None, named({"folded": fo, "unfolded": ~fo, "border": bd, "interior": ~bd}))]
    return [(tap, None, {})]


def errors(g, got, ref):
    """{(entry, class): own-norm L2 error} over the taps present in both."""
    e = {}
    for tap in ref:
        if tap not in got:
            continue
        for name, sl, masks in tap_classes(g, tap):
            a, r = (got[tap], ref[tap]) if sl is None else (got[tap][:, sl], ref[tap][:, sl])
            e[(name, "all")] = A.own_norm_err(a, r)
            for cn, m in masks.items():
                e[(name, cn)] = A.own_norm_err(a[..., m], r[..., m])
        if tap == "gres":
            # the InstanceNorm backward removes, per (image, channel), the mean of g_n and its component along xhat: both terms are far
            # below the bf16 storage noise of a pixel but not of a sum over the plane, so the plane's mean and its component along xhat are
            # classes of their own ([B, 64] numbers each)
            xhat = g.cap["b0.xn"].detach().double()
            a, r = got[tap].detach().double(), ref[tap].detach().double()
            e[(tap, "chan_mean")] = A.own_norm_err(a.mean(dim=(2, 3)), r.mean(dim=(2, 3)))
            e[(tap, "along_xhat")] = A.own_norm_err((a * xhat).mean(dim=(2, 3)), (r * xhat).mean(dim=(2, 3)))
    return e


def stage_errors(g, taps, gpre_ref=None):
    """The gate's measurement of a set of taps (a device run, or the emulation playing one): each tap against the VJP of its own
    upstream taps.  gpre_ref: the seed's reference (``seed``), when the seed itself is gated."""
    refs = stage_refs(g, taps)
    if gpre_ref is not None:
        refs = dict(refs, gpre=gpre_ref)
    return errors(g, taps, refs), refs


def oracle32_errors(g64, g32, taps, refs64, gpre_ref=None):
    """The float32 oracle's own error on the same stages: stage_refs on the float32 graph (same cotangents) against float64."""
    refs32 = stage_refs(g32, taps)
    if gpre_ref is not None:
        refs32["gpre"] = gpre_ref.float()
    return errors(g64, refs32, refs64)


def budget(g, gpre):
    """bf16 error budget {(entry, class): error}: the emulated taps through the gate's own measurement."""
    emu = emulate(g, gpre, points=True)
    return stage_errors(g, emu, gpre_ref=emu["gpre"])[0]


def gate_bf16(err, bud, floor=None):
    """-> (failures, {(entry, class): (error, effective budget, ratio)}).  Effective budget: the emulation's, or the floor (the float32
    oracle's own error) where the emulation's is exactly zero."""
    table, bad = {}, []
    for k, e in err.items():
        b = bud.get(k, 0.0)
        if b == 0.0 and floor is not None:
            b = floor.get(k, 0.0)
        q = e / b if b > 0 else (0.0 if e == 0 else math.inf)
        table[k] = (e, b, q)
        if not e <= A.MARGIN * b:
            bad.append(f"{k[0]}[{k[1]}]: error {e:.3e} > {A.MARGIN:g} x budget {b:.3e} (ratio {q:.2f})")
    return bad, table


def gate_fp32(err, o32):
    """-> (failures, {(entry, class): (error, float32 oracle's error, ratio)}): <= 1e-4 of own norm, or <= 3 x the float32 oracle's error."""
    table, bad = {}, []
    for k, e in err.items():
        o = o32.get(k, 0.0)
        table[k] = (e, o, e / o if o > 0 else (0.0 if e == 0 else math.inf))
        if not (e <= FP32_TOL or e <= A.MARGIN * o):
            bad.append(f"{k[0]}[{k[1]}]: error {e:.3e} > {FP32_TOL:g} and > {A.MARGIN:g} x the float32 oracle's {o:.3e}")
    return bad, table


def format_table(table, third="ratio"):
    return "\n".join(f"    {t:10s} {c:11s} err {e:.3e}  ref {b:.3e}  {third} {q:6.2f}" for (t, c), (e, b, q) in table.items())
