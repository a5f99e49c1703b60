"""Teacher-forced stage gate of the backward pass: fp64 reference per stage, bf16 error budget, per-pixel-class comparator.

Plain helper module (CPU only, no pytest hooks), shared by tests/test_bwd_stage_reference_cpu.py and tests/test_gpu_bwd_stages.py;
the mirror image of the forward stage gate (tests/fwd_stage_ref.py with tests/test_gpu_fwd_stages.py; check_vs_oracle of
tests/test_gpu_baseline_configs.py is its whole-tensor forerunner at the benchmark geometry) and the model-level continuation of tests/attn_ref.py.

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
  <parameter>   every trainable parameter's gradient (fp32, the oracle's shape) under the parameter's own name: what the deferred
                launch_multi_reduce leaves in the flat gradient buffer, read through q.grad of model.named_parameters()
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
``param_refs`` (graph built with leaf_params=True) does the same for the parameter gradients -- VJP from the nearest intact upstream tap to
the parameter leaf, cotangent = the run's own value of that tap; kernels as backward_impl launches them:
  last tail conv weight (tail.6 x4, tail.3 x2 / x3)  srpre -> w, cotangent gpre       fused / streaming tail backward, or launch_final_conv_wgrad
  tail.3.weight / .bias (x4)                         srpre -> ., cotangent gpre       tail backward (g_t2pre in LDS), or launch_wgrad_tn UNSHUF
  tail.0.weight / .bias                              x4: t1pre -> ., cotangent g_t1pre; x2 / x3: srpre -> ., gpre   launch_wgrad_tn UNSHUF / tail_bwd_stream
  body.b.feed_forward.0.weight / .bias               X{b+1} -> ., cotangent gy        conv3x3_c64_bwd_fused / conv3x3_c64_wgrad
  body.b.attn{i}.qkv_conv.weight                     b{b}.qkv{i} -> W, cotangent b{b}.gqkv{i}   launch_wgrad_tn (generic, fast, big tiles)
  body.b.attn{i}.rel_h / .rel_w                      X{b+1} -> ., cotangent gy        attention backward -> rel_reduce1 -> multi_reduce
  head.weight / .bias                                X0 -> ., cotangent gres          launch_wgrad_tn on head_cols
Every one passes through the deferred launch_multi_reduce and its layout modes, so the comparison is elementwise in the oracle's shape.

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
PARAMETER GRADIENTS.  A weight-gradient kernel multiplies the stored bf16 upstream tap by a stored bf16 forward tensor and accumulates in
float32, so a one-kernel stage has NO rounding point: its emulation is the float32 product of those operands (``_gemm_wgrad``,
``_conv_wgrad``) and its budget the float32 accumulation error (the rule for zero-budget entries: the float32 floor).  That holds for the qkv
weights (gqkv x d), the ff conv (gy x xc), tail.0 (g_t1pre x X[n_blocks]) and the bias gradients.  The others carry these points:
  k_tail_bwd.hip / k_conv.hip final_conv_wgrad      "geff"   last tail conv weight: the seed is a bf16 MFMA operand (Geff; from_f<T>(gout))
  k_tail_bwd.hip / k_gemm.hip wgrad_tn UNSHUF       "geff", "gt2"   tail.3 weight and bias (x4): bf16(g(t2)) x stored gelu(t1)
  k_tail_bwd_stream.hip (x2 / x3)                   "geff", "gt1"   tail.0 weight and bias: bf16(g(t)) x X[n_blocks]
  k_conv.hip head_im2col_kernel                     "hcols"  head weight: the reflect-padded INPUT is stored in bf16 for the GEMM (the forward head
                                                             conv reads it in fp32)
  attention backward                                rel-pos tables: "gxc", "do" and the attention's own points; rel_reduce1 and the deferred
                                                    reduction sum the windows in fp32 (no point)
Accumulation orders restated because a correct kernel stood above 3 x a blocked torch float32 sum (as lr.grad did): the BIAS gradients.
They are column sums of bf16 values whose torch float32 sum is exact to a fraction of an ulp (1.4e-8 of own norm at 1x32x32, where the ff
bias stood at 4.8e-8, 3.5x, and tail.0's at 2.4x): restated as the kernels sum them --
  conv3x3_c64_bwd_rows_kernel   a workgroup walks every nblk-th 32-pixel-wide segment of rs rows (launch_conv3x3_c64_bwd_fused's rs, nblk),
                                one MFMA of a row's 32 pixels against ones per row: ONE float32 chain per workgroup (``_bias_chain_conv_bwd``)
  wgrad_tn_kernel               one MFMA of 32 rows against ones per step, one chain per slab (``wgrad_slabs``: slab partition of
                                launch_wgrad_tn), tail.0 (x4) and head bias (``_bias_chain_wgrad_tn``)
  multi_reduce_kernel           the slabs: wave g takes slabs g, g + 4, ..., four partial sums, (a0 + a1) + (a2 + a3), then the four waves
                                (``_slab_reduce``)
The weight gradients themselves stayed within 1.5x of the blocked float32 product in every cell and keep it.
SCATTER OF THE REL-POS BUDGET.  A rel-pos table's gradient is a sum over every window and query with heavy cancellation; its error vector
has few effective degrees of freedom, so the own-norm error of ONE emulation is itself a noisy number: two equally legitimate emulations
(the same chain from the seed times 1.37, or 0.71 -- the mathematics is linear, only the bf16 roundings fall differently) differ by 0.22x ..
3.09x per (table, class) at 1x32x32 and 2x40x56, where every other bf16-sized entry stays within 0.64x .. 1.84x.  Against a budget drawn
that way the device's tables scattered likewise (0.34x .. 3.03x over all cells on MI355X; 3.03x: attn2.rel_w[ring] at 3x64x96, where the
emulation's draw for the ring was 1.8e-3 next to 1.5e-2 for the inner rows).  No margin answers that; the draw has to be the device's.  So
for a device run ``budget(g, gpre, taps)`` restates the tables' stage from the run's OWN gy -- the cotangent their reference takes: the
same chain, the same points, but on the values the device started from, so the roundings fall where the device's fell (an fp32 sum in
another order flips a bf16 rounding once in ~1e4 values) and the two errors are one draw.  When the emulation plays the device this is
the plain budget, bit for bit (tests/test_wgrad_stage_reference_cpu.py).
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
  parameters (``param_classes``)    elementwise in the oracle's shape, whole tensor and: qkv weight -- row blocks q | k | v (the halo overlap-add
                                    reaches k and v only); rel tables -- ring (index 0 and 9) / inner (1..8); 3x3 weights (head, ff, last tail
                                    conv) -- centre / edge / corner taps (border handling shows off-centre only); tail.0 and x4's tail.3 weight
                                    and bias -- phase<k>, the r0 x r0 pixel-unshuffle phases (channel = c r0^2 + phase); other biases -- 'all'
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
    return types.SimpleNamespace(x=xg, p=p, cap=cap, scale=scale, nb=n_blocks, dtype=dtype, B=B, H0=H0, W0=W0, H=H, W=W, ftype=ftype,
                                 leaf_params=leaf_params)


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


def last_conv(scale):
    return "tail.6.weight" if scale == 4 else "tail.3.weight"


def param_refs(g, taps):
    """{parameter name: reference} (g.ftype, the oracle's parameter shape) for every trainable parameter: the VJP from the nearest intact
    upstream tap to the parameter leaf with `taps`' value of that tap as cotangent (the table in the module docstring).  A parameter
    whose cotangent is not in `taps` is left out.  Needs build_graph(..., leaf_params=True)."""
    if not g.leaf_params:
        raise ValueError("param_refs needs build_graph(..., leaf_params=True)")
    c, nb, p = g.cap, g.nb, g.p
    refs = {}

    def put(out, names, tap):
        if tap in taps:
            refs.update(zip(names, _vjp(out, [p[n] for n in names], taps[tap].to(g.ftype))))

    if g.scale == 4:
        put(c["srpre"], ["tail.6.weight", "tail.3.weight", "tail.3.bias"], "gpre")
        put(c["t1pre"], ["tail.0.weight", "tail.0.bias"], "g_t1pre")
    else:
        put(c["srpre"], ["tail.3.weight", "tail.0.weight", "tail.0.bias"], "gpre")
    for b in range(nb - 1, -1, -1):
        pre = f"body.{b}."
        names = [pre + "feed_forward.0.weight", pre + "feed_forward.0.bias"]
        for i in range(1, 5):
            names += [pre + f"attn{i}.rel_h", pre + f"attn{i}.rel_w"]
            put(c[f"b{b}.qkv{i}"], [pre + f"attn{i}.qkv_conv.weight"], f"b{b}.gqkv{i}")
        put(c[f"X{b + 1}"], names, "gT" if b == nb - 1 else "gB")
    put(c["X0"], ["head.weight", "head.bias"], "gres")
    return refs


def autograd_param_grads(g, g_sr, rgb_range=1.0):
    """Every trainable parameter's gradient by plain torch.autograd.grad of sum(clamp(sr) * g_sr) (the consistency test's yardstick)."""
    H0s, W0s = g.H0 * g.scale, g.W0 * g.scale
    loss = (torch.clamp(g.cap["srpre"][..., :H0s, :W0s], 0.0, rgb_range) * g_sr.to(g.ftype)).sum()
    names = O.trainable_names(g.p)
    return dict(zip(names, _vjp(loss, [g.p[n] for n in names], None)))


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
# faults of the parameter gradients alone (every data tap stays as it is): tests/test_wgrad_stage_reference_cpu.py
PARAM_FAULTS = tuple(f"{f}:{i}" for f in ("wgrad_tail_rows", "rel_drop_window", "rel_swap") for i in range(4)) + (
    "bias_one_slab", "tail0_phase_order", "head_wgrad_zero_pad", "ff_wgrad_tap_transposed")


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


def wgrad_slabs(M, N, K):
    """(slabs, rows per slab) of launch_wgrad_tn's 64 x 64-tile bf16 kernels (csrc/k_gemm.hip: generic and fast path)."""
    tn, tk = -(-N // 64), -(-K // 64)
    ns = min(1024, max(1, 512 // (tn * tk)), -(-M // 128))
    if ns > 8:
        ns = ns // 8 * 8
    rps = -(-(-(-M // ns)) // 128) * 128
    return -(-M // rps), rps


def _rows(t):
    """[B, C, h, w] -> [M = B h w, C]: the row order of the weight-gradient GEMMs (NHWC)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _acc(t, f32):
    """The weight-gradient kernels accumulate in float32: with the rounding points on, their products are restated in float32."""
    return t.detach().float() if f32 else t.detach()


def _gemm_wgrad(G, X, f32, shape, keep=None):
    """dW[n][k] = sum_m G[m][n] X[m][k] and db[n] = sum_m G[m][n] over the rows m of two [B, C, h, w] tensors; keep: rows that take part."""
    Gr, Xr = _acc(_rows(G), f32), _acc(_rows(X), f32)
    if keep is not None:
        Gr, Xr = Gr[keep], Xr[keep]
    return (Gr.t() @ Xr).reshape(shape), Gr.sum(0)


def _slab_reduce(slabs):
    """multi_reduce_kernel (csrc/k_pointwise.hip) over float32 slabs [ns, ...]: wave g takes slabs g, g + 4, ... into four (eight, while
    32 slabs remain) partial sums, (a0 + a1) + (a2 + a3) per wave, then (w0 + w1) + (w2 + w3) -- float32 adds in that order."""
    ns, z, waves = slabs.shape[0], torch.zeros_like(slabs[0]), []
    for g in range(4):
        a, b, s = [z.clone() for _ in range(4)], [z.clone() for _ in range(4)], g
        while s + 28 < ns:
            for j in range(4):
                a[j], b[j] = a[j] + slabs[s + 4 * j], b[j] + slabs[s + 16 + 4 * j]
            s += 32
        a = [a[j] + b[j] for j in range(4)]
        while s + 12 < ns:
            a = [a[j] + slabs[s + 4 * j] for j in range(4)]
            s += 16
        while s < ns:
            a[0], s = a[0] + slabs[s], s + 4
        waves.append((a[0] + a[1]) + (a[2] + a[3]))
    return (waves[0] + waves[1]) + (waves[2] + waves[3])


def _mfma_chain(parts):
    """parts [nslab, nstep, n] float64: per slab one float32 accumulator that takes one MFMA's exact 32-term sum per step."""
    acc = torch.zeros(parts.shape[0], parts.shape[2], dtype=torch.float32)
    for s in range(parts.shape[1]):
        acc = (acc.double() + parts[:, s]).float()
    return acc


def _bias_chain_wgrad_tn(G):
    """Bias gradient of wgrad_tn_kernel (csrc/k_gemm.hip): one MFMA of 32 rows of G against ones per step, a sequential float32 chain
    over the rows of a slab, then the deferred reduction over the slabs.  G [B, N, h, w] holds bf16 values."""
    Gr = _rows(G).detach().double()
    M, N = Gr.shape
    ns, rps = wgrad_slabs(M, N, 64)
    pad = torch.zeros(ns * rps - M, N, dtype=Gr.dtype)
    return _slab_reduce(_mfma_chain(torch.cat((Gr, pad)).view(ns, rps // 32, 32, N).sum(2)))


def _bias_chain_conv_bwd(gy):
    """Bias gradient of conv3x3_c64_bwd_rows_kernel (csrc/k_conv.hip): a workgroup walks every nblk-th segment (32 pixels wide, rs rows,
    launch_conv3x3_c64_bwd_fused) row by row, one MFMA of the row's 32 pixels against ones per row, one float32 chain per workgroup;
    then the deferred reduction over the workgroups' slabs."""
    B, C, H, W = gy.shape
    strips, rs = B * (W // 32), 64
    while rs > 16 and (H % rs or strips * (H // rs) < 256):
        rs >>= 1
    nseg, nsx = H // rs, W // 32
    nsegs = strips * nseg
    nblk = min(256, nsegs)
    # segment sg = (b, strip sx, rows seg): [nsegs, rs, C] exact sums over the 32 pixels of a row
    P = gy.detach().double().view(B, C, nseg, rs, nsx, 32).sum(5).permute(0, 4, 2, 3, 1).reshape(nsegs, rs, C)
    rounds = -(-nsegs // nblk)
    P = torch.cat((P, torch.zeros(rounds * nblk - nsegs, rs, C, dtype=P.dtype))).view(rounds, nblk, rs, C)
    return _slab_reduce(_mfma_chain(P.permute(1, 0, 2, 3).reshape(nblk, rounds * rs, C)))


def _conv_wgrad(x, gout, wshape, mode, f32):
    """Weight and bias gradient of conv3x3(pad_1(x)) for the output gradient gout; mode: the ring, 'reflect' or 'constant' (zeros)."""
    x, gout = _acc(x, f32), _acc(gout, f32)
    w = torch.zeros(wshape, dtype=x.dtype, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(F.pad(x, (1, 1, 1, 1), mode=mode), w), w, gout)
    return gw, gout.sum((0, 2, 3))


def _emulate_tail(g, gpre, pts, fault):
    c, s = g.cap, g.scale
    fold = fault != "tail_no_reflect"
    last = last_conv(s)
    a_last = c["t2act" if s == 4 else "t1act"]
    ga = _reflect_conv_adjoint(_rnd(gpre, pts), _w(g, last, True), a_last.shape, fold)
    out = {}
    # the last conv's weight gradient takes the bf16 seed ("geff") and the stored (or recomputed: same bits) bf16 activation
    out[last], _ = _conv_wgrad(a_last, _rnd(gpre, pts), g.p[last].shape, "reflect", pts)
    if s == 4:
        gt2 = _rnd(ga * c["t2der"].detach(), pts)
        out["tail.3.weight"], out["tail.3.bias"] = _gemm_wgrad(F.pixel_unshuffle(gt2, 2), c["t1act"], pts, g.p["tail.3.weight"].shape)
        ga1 = F.conv_transpose2d(F.pixel_unshuffle(gt2, 2), _w(g, "tail.3.weight", True))
        gt1 = out["g_t1pre"] = _rnd(ga1 * c["t1der"].detach(), pts)
        r0 = 2
    else:
        gt1 = _rnd(ga * c["t1der"].detach(), pts)
        r0 = s
    gu, Y = F.pixel_unshuffle(gt1, r0), c[f"X{g.nb}"]
    wT, bT = _gemm_wgrad(gu, Y, pts, g.p["tail.0.weight"].shape)
    if pts and s == 4:                               # (x2 / x3: the streaming tail kernel's own sums, float32 as restated above)
        bT = _bias_chain_wgrad_tn(gu)
    if fault == "bias_one_slab":                     # tail.0's bias gradient from the rows of slab 0 alone
        M = gu.shape[0] * gu.shape[2] * gu.shape[3]
        _, bT = _gemm_wgrad(gu, Y, pts, g.p["tail.0.weight"].shape, keep=torch.arange(M) < wgrad_slabs(M, gu.shape[1], 64)[1])
    if fault == "tail0_phase_order":                 # sub-pixel (dy, dx) stored where (dx, dy) belongs
        perm = torch.arange(64 * r0 * r0).view(64, r0, r0).transpose(1, 2).reshape(-1)
        wT, bT = wT[perm], bT[perm]
    out["tail.0.weight"], out["tail.0.bias"] = wT, bT
    out["gT"] = _rnd(F.conv_transpose2d(gu, _w(g, "tail.0.weight", True)), pts)
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
    ffw, out[pre + "feed_forward.0.bias"] = _conv_wgrad(c[f"b{b}.xc"], gy, g.p[pre + "feed_forward.0.weight"].shape, "constant", pts)
    if pts:
        out[pre + "feed_forward.0.bias"] = _bias_chain_conv_bwd(gy)
    out[pre + "feed_forward.0.weight"] = ffw.transpose(2, 3) if fault == "ff_wgrad_tap_transposed" else ffw
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
        apts = A.kernel_points(C) if pts else (A.POINTS_ORACLE_EMU if g.dtype == "bf16" else frozenset())
        ex = A.explicit(inp, apts, dtype=g.ftype)
        out[f"b{b}.drel{i + 1}"] = (ex["drel_h"], ex["drel_w"])
        gqkv = out[f"b{b}.gqkv{i + 1}"] = torch.cat((ex["dq"], ex["dk"], ex["dv"]), dim=1)
        # parameter gradients of the branch: the rel-pos tables come out of the attention backward (rel_reduce1 and the deferred
        # reduction sum the windows in fp32), the qkv weight is one GEMM of the stored gqkv with the stored branch input d
        drh, drw = ex["drel_h"], ex["drel_w"]
        if fault == f"rel_drop_window:{i}":            # the last window's share missing from the sum over windows (a window whose dO is
            gl = A.to_windows(inp["gout"]).clone()     # zero has dS = 0 and adds nothing to drel)
            gl[-1] = 0.0
            ex1 = A.explicit(dict(inp, gout=A.from_windows(gl, B, h, w)), apts, dtype=g.ftype)
            drh, drw = ex1["drel_h"], ex1["drel_w"]
        if fault == f"rel_swap:{i}":
            drh, drw = drw, drh
        out[pre + f"attn{i + 1}.rel_h"], out[pre + f"attn{i + 1}.rel_w"] = drh.reshape(1, A.KWIN, 1, C // 2), drw.reshape(1, 1, A.KWIN, C // 2)
        M, keep = B * h * w, None
        if fault == f"wgrad_tail_rows:{i}":            # the last partial 128-row step, or else the last slab, never accumulated
            ns, rps = wgrad_slabs(M, 3 * C, C)
            keep = torch.arange(M) < (M - M % 128 if M % 128 else (ns - 1) * rps)
        wname = pre + f"attn{i + 1}.qkv_conv.weight"
        out[wname], _ = _gemm_wgrad(gqkv, c[f"b{b}.d{i + 1}"], pts, g.p[wname].shape, keep)
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
    """Every tap and every trainable parameter's gradient (under the parameter's name, in its shape) by the explicit chain from the seed
    `gpre`; points: the bf16 round trips of the module docstring; fault: one of FAULTS or PARAM_FAULTS."""
    if fault is not None and fault not in FAULTS + PARAM_FAULTS:
        raise ValueError(fault)
    gpre = gpre.to(g.ftype)
    out = {"gpre": gpre}
    out.update(_emulate_tail(g, gpre, points, fault))
    gy = out["gT"]
    for b in range(g.nb - 1, -1, -1):
        gy = _emulate_block(g, b, gy, out["gT"], points, fault, out)
        out["gres" if b == 0 else "gB"] = gy
    # head: launch_wgrad_tn on head_cols, the im2col of the reflect-padded input, which bf16 mode stores in bf16 ("hcols")
    xin = O.pad_to_multiple(g.x.detach())
    out["head.weight"], out["head.bias"] = _conv_wgrad(_rnd(xin, points and g.dtype == "bf16"), gy, g.p["head.weight"].shape,
                                                       "constant" if fault == "head_wgrad_zero_pad" else "reflect", points)
    if points:
        out["head.bias"] = _bias_chain_wgrad_tn(gy)
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


def param_classes(g, name):
    """{class: bool mask in the parameter's own shape} for one trainable parameter (module docstring, COMPARATOR)."""
    shp = tuple(g.p[name].shape)

    def full(m):
        return m.expand(shp)
    if name.endswith("qkv_conv.weight"):
        row = torch.arange(shp[0]).view(-1, 1, 1, 1) // shp[1]
        return {n: full(row == k) for k, n in enumerate("qkv")}
    if name.endswith(("rel_h", "rel_w")):
        idx = torch.arange(A.KWIN).view((1, A.KWIN, 1, 1) if name.endswith("rel_h") else (1, 1, A.KWIN, 1))
        ring = (idx == 0) | (idx == A.KWIN - 1)
        return {"ring": full(ring), "inner": full(~ring)}
    if len(shp) == 4 and shp[2:] == (3, 3):
        off = (torch.arange(3).view(3, 1) != 1).long() + (torch.arange(3).view(1, 3) != 1).long()       # 0 centre, 1 edge, 2 corner
        return {n: full((off == k).view(1, 1, 3, 3)) for k, n in enumerate(("centre", "edge", "corner"))}
    if name.startswith("tail."):                  # a pixel-shuffled expansion: output channel = c r0^2 + sub-pixel phase
        r2 = (2 if g.scale == 4 else g.scale) ** 2
        ph = (torch.arange(shp[0]) % r2).view((-1,) + (1,) * (len(shp) - 1))
        return {f"phase{k}": full(ph == k) for k in range(r2)}
    return {}


def errors(g, got, ref):
    """{(entry, class): own-norm L2 error} over the taps and parameter gradients present in both."""
    e = {}
    for tap in ref:
        if tap not in got:
            continue
        if tap in g.p:
            a, r = got[tap].detach().reshape(ref[tap].shape), ref[tap].detach()
            e[(tap, "all")] = A.own_norm_err(a, r)
            for cn, m in param_classes(g, tap).items():
                e[(tap, cn)] = A.own_norm_err(a[m], r[m])
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
    if g.leaf_params:
        refs.update(param_refs(g, taps))
    if gpre_ref is not None:
        refs = dict(refs, gpre=gpre_ref)
    return errors(g, taps, refs), refs


def oracle32_errors(g64, g32, taps, refs64, gpre_ref=None):
    """The float32 oracle's own error on the same stages: stage_refs on the float32 graph (same cotangents) against float64."""
    refs32 = stage_refs(g32, taps)
    if g32.leaf_params:
        refs32.update(param_refs(g32, taps))
    if gpre_ref is not None:
        refs32["gpre"] = gpre_ref.float()
    return errors(g64, refs32, refs64)


def budget(g, gpre, taps=None):
    """bf16 error budget {(entry, class): error}: the emulated taps through the gate's own measurement.
    taps (a device run's): the rel-pos tables' stage is then emulated from the RUN'S OWN gy, the cotangent their reference takes, instead
    of the emulated one -- the block's chain (conv data gradient, the branch chain, the attention backward and its points) restated on
    the values the device started from, so that the emulation's roundings fall where the device's do and both errors are the same draw
    (module docstring, SCATTER OF THE REL-POS BUDGET).  With the emulation's own taps this changes nothing: budget(g, gpre, emu) ==
    budget(g, gpre)."""
    emu = emulate(g, gpre, points=True)
    bud = stage_errors(g, emu, gpre_ref=emu["gpre"])[0]
    if taps is not None and g.leaf_params:
        for b in range(g.nb - 1, -1, -1):
            names = [f"body.{b}.attn{i}.rel_{a}" for i in range(1, 5) for a in "hw"]
            gy = taps["gT" if b == g.nb - 1 else "gB"].to(g.ftype)
            out = {}
            _emulate_block(g, b, gy, taps["gT"].to(g.ftype), True, None, out)
            refs = dict(zip(names, _vjp(g.cap[f"X{b + 1}"], [g.p[n] for n in names], gy)))
            bud.update(errors(g, {n: out[n] for n in names}, refs))
    return bud


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
