"""Stage gate of the forward pass: fp64 reference per stage, bf16 error budget, per-pixel-class comparator.

Plain helper module (CPU only, no pytest hooks), shared by tests/test_fwd_stage_reference_cpu.py and tests/test_gpu_fwd_stages.py; the
mirror image of the backward stage gate (tests/bwd_stage_ref.py) and the model-level continuation of tests/attn_ref.py.  The whole-tensor
check_vs_oracle of tests/test_gpu_baseline_configs.py stays: it ties the benchmark geometry (square, unpadded) to the oracle.

STAGES.  One stage is one launch of the default schedule (m2t_forward in csrc/m2t_api.hip), evaluated from the run's OWN stored upstream
tensors -- tests/gpu_util.hip_forward_trace plus the input -- so a stage carries one kernel's worth of error and nothing of the network's
amplification (oracle/m2trans_oracle.py, the note on bf16 emulation):
  X0                 lr: reflect pad to the multiple of 32 (right / bottom), head conv on fp32 weights, reflect ring
  b.mean, b.rstd     X_b: biased variance, eps 1e-5 ([B, 64], fp32 in both compute types)
  b.d_i              X_b and, for i >= 2, b.xc[16 (i - 2) : 16 (i - 1)]: norm chunk i, mix xin_i = (xn_i + x_{i-1}) / 2 (i = 1: xin_1 = xn_1), DWT^L
  b.qkv_i            b.d_i, where q | k | v is stored: always for i = 3, 4; for i = 1, 2 in fp32 and with fused_c16_fwd / fused_attn_fwd = 0 / 1
  b.xc[16 (i-1):16 i]  b.qkv_i -- or b.d_i where the fused kernel does not store q | k | v: the stage is then the whole fused kernel with the
                     qkv rounding inside it as a point -- attention, IWT^L, + xin_i.  The residual xin_i is restated from X_b and the previous
                     slice exactly as the b.d_i stage does (the workspace's xin scratch is overwritten by the next branch)
  X_{b+1}            b.xc, X_b, and X0 in the last block (`res + x` folded into the conv's epilogue): zero-padded 3x3 conv + bias + residuals
  t1act, t1der       X_nb: tail.0, pixel shuffle (r = 2 for x4, else the scale), GELU and GELU'
  t2act, t2der (x4)  t1act: tail.3, pixel shuffle 2, GELU and GELU'
  srpre              the last stored activation (t2act for x4, else t1act): reflect-padded 3x3 conv, fp32 output at the padded size
  sr                 srpre: clamp to [0, R] and crop to [H0 s, W0 s]
The default bf16 tails keep the last GELU in LDS or registers; tests/test_gpu_fwd_stages.py takes t2act / t1act from the stored-form run,
whose sr is bit-equal.  Inference plans and local_norm store no stage and are out of scope (their bit-identity with the training
plan's forward: tests/test_gpu_lean_inference.py, tests/test_gpu_local_norm.py), and so are maps of >= 0.5 M pixels, where the rows conv
takes segments of 32 or 64 rows (tests/test_gpu_baseline_configs.py test_config4 covers length 32 on whole tensors).

REFERENCE.  ``reference(g, taps)``: every stage in float64 with no rounding anywhere -- fp32 master weights, exact erf GELU, exact softmax --
from `taps`' value of its upstream tensors.  ``reference(g, chain=True)`` feeds each stage the previous stage's reference instead and
reproduces oracle.m2trans_oracle.forward in float64 (tests/test_fwd_stage_reference_cpu.py: 1e-12).  ``oracle32`` is the same in float32:
the float32 oracle's own error, the floor of zero budgets and the fp32 gate's yardstick.

BUDGET.  ``emulate(g, taps)`` is the same stage in float32 with a value -> bf16 -> value round trip wherever the default bf16 schedule holds a
bf16 value, on the run's own inputs of that stage, so that the roundings fall where the device's fell (the rule bwd_stage_ref.budget
arrived at).  The budget of a (stage, class) is the emulation's error against the reference.  Only this arithmetic feeds a budget;
nothing from a HIP run does.  ROUNDING POINTS, per kernel (every accumulation, the statistics, the softmax, the Haar butterflies, bias
and residual adds are fp32 and are no points; a residual is read as the stored bf16 value):
  k_pointwise.hip pack_kernel                         "w"      every packed weight: qkv, feed_forward.0, tail.0, tail.3 (x4); the last tail conv's
                                                               weight is rounded when it is staged (k_conv.hip, k_tail*.hip); head: fp32
  k_conv.hip      head_conv_fwd_kernel                "X0"     the stored output alone (fp32 input, fp32 weights)
  k_pointwise.hip instnorm_stats1 / 2, instnorm_finalize   --  no point; ACCUMULATION ORDER restated in float32 (``_stats_emulated``): per thread a
                                                               two-pass (mean, squared deviations) over <= 16 values, Welford / Chan merges of
                                                               (n, mean, M2) per thread, workgroup and over the 32 splits in the kernels' tree;
                                                               blocks >= 1 of the bf16 rows conv: 256-value partials of the STORED output from the
                                                               conv's epilogue (k_conv.hip stat_flush), merged by instnorm_finalize_kernel
  k_attn_c16.hip  window_attn_fused_c16_fwd           "d"      d1 = bf16(xn_1);  "qkv" in registers / LDS;  attn_ref.kernel_points "khat", "p";
                                                      "xc"     the stored slice bf16(attention + d1)
  k_pointwise.hip branch_prep(_tiled)_kernel,         "xin"    the mixed branch input bf16((xn_i + x_{i-1}) / 2), stored AND transformed as stored
  k_attn_fused.hip / k_attn_fwd2.hip prep phase       "d"      the stored d_i = bf16(DWT^L(xin_i))
  k_gemm.hip gemm_nt / the fused kernels' projection  "qkv"    bf16(d W^T): stored, or held in LDS by the fused kernels
  k_attn_res.hip, k_attn_fused.hip, k_attn_fwd2.hip   "khat", "p" of attn_ref.kernel_points;  "xc": bf16(IWT^L(P V) + xin_i) -- the attention output
                                                               itself stays fp32 through the inverse butterflies (no "out" point here)
  k_conv.hip      conv3x3_c64_rows / _pipe / tile     "X"      the stored block output: + bias + X_b (+ X0), ONE rounding
  k_gemm.hip      tail_expand_kernel,                 "act", "der"   gelu_fast_both (csrc/m2t_common.h) of the fp32 pre-activation, both stored in bf16
  k_tail_fwd*.hip (LDS / registers)                            (the approximation is restated, as O._gelu_stored does: the gate measures the kernels)
  k_conv.hip final_conv_fwd / the fused tails         --       srpre is fp32: the rounded weight is the stage's only point
  k_pointwise.hip clamp_l1                            --       exact: budget zero, sr must be bit-equal to clamp(srpre) cropped
The first device run forced no further rounding point or accumulation order into the emulation.

COMPARATOR.  ``errors``: own-norm L2 error || got - ref || / || ref || over the whole tensor ('all') and per class:
  X0                  border / interior of the padded plane; pad (rows and columns the reflect pad added) / image
  b.d_i, b.qkv_i      attn_ref.pixel_classes 'kv' at the branch's level (img_border, cover1 / 2 / 4); pad / image (a level-L pixel is `image`
                      when its block's first pixel is)
  b.xc[i]             image-corner / image-edge / interior WINDOWS of the branch's level (attn_ref 'q' classes, a full-resolution pixel takes
                      the class of its level-L coordinate): the number of phantom keys differs; pad / image
  X_{b+1}             border / interior (this conv is zero-padded)
  t*act, t*der, srpre border / interior (the tail conv is reflect-padded); srpre also crop / outside
  chan_mean           every stage but mean, rstd and sr: the [B, C] per-plane means of got and ref, || mean(got) - mean(ref) || over the norm
                      of the reference's per-plane RMS.  A systematic bias (truncation instead of round-to-nearest, a statistics error that
                      moves a whole plane) is far below a pixel's bf16 noise but not below that of a plane's mean.  The denominator is the
                      planes' RMS, not their mean: the planes of d_1 and qkv_1 have mean zero by construction (InstanceNorm's output), and
                      the ratio error / budget does not depend on the denominator
  b.mean, b.rstd, sr  'all' only
GATES.  bf16 (``gate_bf16``): every entry <= attn_ref.MARGIN (3) x its budget; where a budget is exactly zero (sr) the floor is the float32
oracle's own error on that stage, zero as well: sr must be bit-equal, in both compute types (``gate_fp32`` asks the same).  fp32: every
entry <= attn_ref.FP32_TOL["out"] = 2e-5, or <= 3 x the float32 oracle's error (the rule check_vs_oracle applies).  The margin is not a knob:
a correct kernel that exceeds it has a rounding point or an accumulation order that is missing above.

FAULTS.  Deliberately wrong variants of the emulation (tests/test_fwd_stage_reference_cpu.py: each one is flagged):
  trunc:X1            the block output truncated to bf16 instead of rounded to nearest   (chan_mean; 'all' stands at 2x)
  phantom_no_rel:i    branch i + 1: a phantom key (zero padding of k | v) without its rel-pos term.  A SECOND-ORDER fault at stage level: the
                      phantom keys carry V = 0, so only their share of the softmax mass moves.  With the closed-form weights (logits of
                      ~0.5) that is a quarter of a pixel's bf16 noise in the slice (1.11x the budget in the corner windows at 1x40x56) and
                      this gate does NOT see it; the operator gate does (tests/test_gpu_attn_ops.py, regime kzero).  It is flagged here,
                      through chan_mean, from closed_form_params(gain = 2) on: four times the logits
  haar_sign:1         branch 2: the second Haar sub-band of d with its sign flipped
  no_half:2           branch 3: the mix without the / 2
  pad_replicate       replicate instead of reflect in the rows and columns pad_to_multiple adds
  stats_unpadded      InstanceNorm statistics over the unpadded [H0, W0] region only
  last_conv_zero_pad  zero instead of reflect padding in the last tail conv
  shuffle_hw_swap     tail.0's pixel shuffle with the row pitch taken from H instead of W: invisible at H = W
  crop_corner         sr cropped at the bottom-right corner of the padded output instead of the top-left one
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
FP32_TOL = A.FP32_TOL["out"]
EPS = 1e-5                      # InstanceNorm (oracle.m2trans_oracle.instance_norm)
NORM_SPLIT = 32                 # M2T_NORM_SPLIT (csrc/m2t_common.h)

FAULTS = ("trunc:X1", "phantom_no_rel:0", "phantom_no_rel:1", "haar_sign:1", "no_half:2", "pad_replicate", "stats_unpadded",
          "last_conv_zero_pad", "shuffle_hw_swap", "crop_corner")


# ------------------------------------------------------------------------------------------------ geometry
def geometry(x, params, scale, n_blocks, dtype, stored_qkv=None, conv_stats=None, rgb_range=1.0):
    """The cell: input, fp32 master weights, sizes.  stored_qkv: the branches (1..4) whose q | k | v the run stores (default: all in fp32,
    3 and 4 in bf16); conv_stats: blocks >= 1 take their statistics from the rows conv's epilogue (default: bf16)."""
    B, _, H0, W0 = x.shape
    H, W = O.pad_to_multiple(x).shape[-2:]
    if stored_qkv is None:
        stored_qkv = (1, 2, 3, 4) if dtype == "fp32" else (3, 4)
    if conv_stats is None:
        conv_stats = dtype == "bf16"
    return types.SimpleNamespace(x=x.detach().float(), p={k: v.detach().float() for k, v in params.items()}, scale=scale, nb=n_blocks,
                                 dtype=dtype, B=B, H0=H0, W0=W0, H=H, W=W, stored_qkv=tuple(stored_qkv), conv_stats=bool(conv_stats),
                                 rgb_range=rgb_range)


def last_act(scale):
    return "t2act" if scale == 4 else "t1act"


def last_conv(scale):
    return "tail.6.weight" if scale == 4 else "tail.3.weight"


# ------------------------------------------------------------------------------------------------ pieces of a stage
def _rnd(x, on=True):
    return A.bf16_round(x) if on else x


def _trunc(x):
    """value -> bf16 by truncation (the fault): the low 16 bits of the float32 pattern dropped."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


def _dwt_l(x, L):
    for _ in range(L):
        x = O.dwt(x)
    return x


def _iwt_l(x, L):
    for _ in range(L):
        x = O.iwt(x)
    return x


def _wf_merge(a, b):
    """wf_merge of csrc/k_pointwise.hip on float32 tensors (n, mean, M2); an empty side leaves the other one as it is."""
    n = a[0] + b[0]
    f = torch.where(n > 0, b[0] / n.clamp(min=1.0), torch.zeros_like(n))
    d = torch.where(b[0] > 0, b[1] - a[1], torch.zeros_like(n))
    return n, a[1] + d * f, a[2] + b[2] + d * d * a[0] * f


def _finish(n, mean, m2):
    return mean, 1.0 / torch.sqrt(m2 / n + EPS)


def _stats_two_stage(X):
    """instnorm_stats1_kernel + instnorm_stats2_kernel in float32: split s of 32 holds ceil(P / 32) consecutive pixels, lane l of 32 every
    32nd of them, 16 at a time (two-pass, then one Welford merge); the lanes merge as N, sum n mean / N, sum (M2 + n (mean - mean_b)^2);
    the splits by the fixed pairwise tree."""
    B, C, H, W = X.shape
    P = H * W
    x = X.float().reshape(B, C, P)
    per = -(-P // NORM_SPLIT)
    ngrp = max(1, -(-per // 512))
    idx = (torch.arange(NORM_SPLIT).view(-1, 1, 1, 1) * per + torch.arange(32).view(1, -1, 1, 1)
           + 512 * torch.arange(ngrp).view(1, 1, -1, 1) + 32 * torch.arange(16).view(1, 1, 1, -1))
    end = ((torch.arange(NORM_SPLIT) + 1) * per).clamp(max=P).view(-1, 1, 1, 1)
    ok = (idx < end).float()
    v = x[:, :, idx.clamp(max=P - 1)] * ok                                 # [B, C, split, lane, group, 16]
    cnt = ok.sum(-1)
    mean = v.sum(-1) * (1.0 / cnt.clamp(min=1.0))
    m2 = (((v - mean.unsqueeze(-1)) * ok) ** 2).sum(-1)
    cnt = cnt.expand_as(mean)
    z = torch.zeros_like(mean[..., 0])
    w = (z, z, z)
    for gi in range(ngrp):
        w = _wf_merge(w, (cnt[..., gi], mean[..., gi], m2[..., gi]))
    N = w[0].sum(-1)                                                       # [B, C, split]
    mean_b = (w[0] * w[1]).sum(-1) / N.clamp(min=1.0)
    dev = (w[2] + w[0] * (w[1] - mean_b.unsqueeze(-1)) ** 2).sum(-1)
    parts = [(N[..., s], mean_b[..., s], dev[..., s]) for s in range(NORM_SPLIT)]
    step = 1
    while step < NORM_SPLIT:
        for s in range(0, NORM_SPLIT, 2 * step):
            parts[s] = _wf_merge(parts[s], parts[s + step])
        step *= 2
    return _finish(*parts[0])


def _stats_conv_epilogue(X):
    """The partials conv3x3_c64_rows_kernel<.., ST = true> leaves (stat_flush: per 32-pixel strip, 16-row group and row parity one (256, mean,
    M2) of the STORED values; a lane's 16 values first, then the 16 lanes with equal counts) and instnorm_finalize_kernel over them."""
    B, C, H, W = X.shape
    x = X.float().view(B, C, H // 16, 8, 2, W // 32, 16, 2)                # rows = (group, row in wave, parity), columns = (strip, lane, 2)
    x = x.permute(0, 1, 2, 4, 5, 6, 3, 7).reshape(B, C, -1, 16, 16)        # [B, C, partial, lane, 16 values]
    mean_l = x.mean(-1)
    m2_l = ((x - mean_l.unsqueeze(-1)) ** 2).sum(-1)
    mean_w = mean_l.mean(-1)
    m2_w = (m2_l + 16.0 * (mean_l - mean_w.unsqueeze(-1)) ** 2).sum(-1)
    n = torch.full_like(mean_w, 256.0)
    N = n.sum(-1)
    mu = (n * mean_w).sum(-1) / N
    M2 = (m2_w + n * (mean_w - mu.unsqueeze(-1)) ** 2).sum(-1)
    return _finish(N, mu, M2)


def _stats(g, X, b, mode, fault):
    if fault == "stats_unpadded":
        X = X[..., :g.H0, :g.W0]
    if mode != "emu":
        mu = X.mean(dim=(2, 3))
        return mu, 1.0 / torch.sqrt(X.var(dim=(2, 3), unbiased=False) + EPS)
    if b > 0 and g.conv_stats and g.dtype == "bf16" and fault != "stats_unpadded":
        return _stats_conv_epilogue(X)
    return _stats_two_stage(X)


def _attention(q, k, v, rel_h, rel_w, pts, no_phantom_rel=False):
    """O.window_attention_core restated on attn_ref's window helpers, with the forward points of attn_ref.kernel_points (khat, p)."""
    B, C, h, w = q.shape
    qw, kw, vw = A.to_windows(q), A.to_key_windows(k), A.to_key_windows(v)
    bias = A.rel_bias(rel_h.reshape(A.KWIN, C // 2), rel_w.reshape(A.KWIN, C // 2)).to(q.dtype)
    if no_phantom_rel:
        bias = bias * A.to_key_windows(torch.ones(B, 1, h, w, dtype=q.dtype))
    kh = _rnd(kw + bias, pts)
    S = torch.bmm(qw, kh.transpose(1, 2)) * (float(C) ** -0.5)
    P = _rnd(torch.softmax(S, dim=-1), pts)
    return A.from_windows(torch.bmm(P, vw), B, h, w)


def _shuffle(t, r, swap):
    """F.pixel_shuffle; swap (the fault): the input's pixel index decomposed with H as the row pitch."""
    if not swap:
        return F.pixel_shuffle(t, r)
    B, C, H, W = t.shape
    return F.pixel_shuffle(t.reshape(B, C, W, H), r).reshape(B, C // (r * r), H * r, W * r)


# ------------------------------------------------------------------------------------------------ the stages
def _run(g, taps, mode, fault=None, chain=False):
    """Every stage output.  mode: 'ref' float64, no rounding; 'f32' float32, no rounding; 'emu' float32 with the rounding points of the
    module docstring when g.dtype is bf16.  chain: each stage takes the previous stage's OUTPUT instead of `taps`' value."""
    if fault is not None and fault not in FAULTS:
        raise ValueError(fault)
    ft = torch.float64 if mode == "ref" else torch.float32
    pts = mode == "emu" and g.dtype == "bf16"
    p, s, nb = g.p, g.scale, g.nb
    out = {}

    def up(name):
        return (out[name] if chain else taps[name]).to(ft)

    def store(t, name=None):
        if pts and name is not None and fault == "trunc:" + name:
            return _trunc(t)
        return _rnd(t, pts)

    def wt(name):                                   # a packed weight
        return _rnd(p[name].to(ft), pts)

    x = g.x.to(ft)
    if fault == "pad_replicate":
        xp = F.pad(x, (0, g.W - g.W0, 0, g.H - g.H0), mode="replicate")
    else:
        xp = O.pad_to_multiple(x)
    out["X0"] = store(O.conv3x3_reflect(xp, p["head.weight"].to(ft), p["head.bias"].to(ft)))
    for b in range(nb):
        pre, ck = f"body.{b}.", f"b{b}."
        X = up(f"X{b}")
        mu, rstd = _stats(g, X, b, mode, fault)
        out[ck + "mean"], out[ck + "rstd"] = mu, rstd
        xn = (X - mu.view(g.B, 64, 1, 1)) * rstd.view(g.B, 64, 1, 1)           # (q - mu) * rs, as branch_prep applies it
        slices = []
        for i in range(4):
            C, L = BR_C[i], BR_L[i]
            xn_i = xn[:, 16 * i:16 * i + 16]
            if i == 0:
                xin = d = store(xn_i)
            else:
                xprev = slices[i - 1] if chain else taps[ck + "xc"][:, 16 * (i - 1):16 * i].to(ft)
                xin = store(xn_i + xprev if fault == f"no_half:{i}" else (xn_i + xprev) * 0.5)
                d = _dwt_l(xin, L)
                if fault == f"haar_sign:{i}":
                    d = d.clone()
                    d[:, C // 4:C // 2] *= -1.0
                d = store(d)
            out[ck + f"d{i + 1}"] = d
            qkv = store(F.conv2d(up(ck + f"d{i + 1}"), wt(pre + f"attn{i + 1}.qkv_conv.weight")))
            if (i + 1) in g.stored_qkv:
                out[ck + f"qkv{i + 1}"] = qkv
                qkv = up(ck + f"qkv{i + 1}")
            q, k, v = torch.chunk(qkv, 3, dim=1)
            a = _attention(q, k, v, p[pre + f"attn{i + 1}.rel_h"].to(ft), p[pre + f"attn{i + 1}.rel_w"].to(ft), pts,
                           no_phantom_rel=(fault == f"phantom_no_rel:{i}"))
            slices.append(store(_iwt_l(a, L) + xin))
        out[ck + "xc"] = torch.cat(slices, dim=1)
        y = F.conv2d(up(ck + "xc"), wt(pre + "feed_forward.0.weight"), p[pre + "feed_forward.0.bias"].to(ft), padding=1) + X
        if b == nb - 1:
            y = y + up("X0")
        out[f"X{b + 1}"] = store(y, f"X{b + 1}")

    def expansion(src, wname, bname, r, act, der, swap=False):
        t = _shuffle(F.conv2d(src, wt(wname), p[bname].to(ft)), r, swap)
        a, d = O.gelu_fast_both(t) if pts else (F.gelu(t), O.gelu_derivative(t))
        out[act], out[der] = store(a), store(d)

    expansion(up(f"X{nb}"), "tail.0.weight", "tail.0.bias", 2 if s == 4 else s, "t1act", "t1der", swap=(fault == "shuffle_hw_swap"))
    if s == 4:
        expansion(up("t1act"), "tail.3.weight", "tail.3.bias", 2, "t2act", "t2der")
    a_last, w_last = up(last_act(s)), wt(last_conv(s))
    if fault == "last_conv_zero_pad":
        out["srpre"] = F.conv2d(a_last, w_last, padding=1)
    else:
        out["srpre"] = O.conv3x3_reflect(a_last, w_last)
    cl = torch.clamp(up("srpre"), 0.0, g.rgb_range)
    if fault == "crop_corner":
        out["sr"] = cl[:, :, cl.shape[2] - g.H0 * s:, cl.shape[3] - g.W0 * s:]
    else:
        out["sr"] = cl[:, :, :g.H0 * s, :g.W0 * s]
    return out


def reference(g, taps=None, chain=False):
    """{stage: float64 reference} from `taps`' upstream values; chain=True (taps not needed): from the previous stage's reference."""
    return _run(g, taps, "ref", chain=chain or taps is None)


def oracle32(g, taps):
    """The same stages in float32 without a rounding point: the float32 oracle's own error is errors(g, oracle32, reference)."""
    return _run(g, taps, "f32")


def emulate(g, taps=None, fault=None):
    """The stages in float32 with the bf16 rounding points of the module docstring.  taps given: each stage from `taps`' upstream values (the
    budget of a device run); taps None: chained from the input -- a complete set of taps, the emulation playing the device.
    fault: one of FAULTS."""
    return _run(g, taps, "emu", fault=fault, chain=taps is None)


# ------------------------------------------------------------------------------------------------ comparator
def _border(h, w):
    y, x = torch.arange(h).view(h, 1).expand(h, w), torch.arange(w).view(1, w).expand(h, w)
    return (y == 0) | (y == h - 1) | (x == 0) | (x == w - 1)


def _inside(h, w, h0, w0):
    y, x = torch.arange(h).view(h, 1).expand(h, w), torch.arange(w).view(1, w).expand(h, w)
    return (y < h0) & (x < w0)


def _named(d):
    return {n: m for n, m in d.items() if bool(m.any())}


def _up(m, L):
    return m.repeat_interleave(1 << L, 0).repeat_interleave(1 << L, 1)


def stage_classes(g, name):
    """[(entry, channel slice or None, {class: bool [h, w]}, with chan_mean)] for one stage output."""
    H, W, s = g.H, g.W, g.scale
    base = name.split(".")[-1]
    if base in ("mean", "rstd") or name == "sr":
        return [(name, None, {}, False)]
    if name == "X0":
        bd, im = _border(H, W), _inside(H, W, g.H0, g.W0)
        return [(name, None, _named({"border": bd, "interior": ~bd, "pad": ~im, "image": im}), True)]
    if base[0] == "d" or base.startswith("qkv"):
        L = BR_L[int(base[-1]) - 1]
        h, w = H >> L, W >> L
        im = _inside(h, w, -(-g.H0 // (1 << L)), -(-g.W0 // (1 << L)))
        return [(name, None, dict(A.pixel_classes(h, w)["kv"], **_named({"pad": ~im, "image": im})), True)]
    if base == "xc":
        im = _inside(H, W, g.H0, g.W0)
        res = []
        for i in range(4):
            L = BR_L[i]
            cls = {n: _up(m, L) for n, m in A.pixel_classes(H >> L, W >> L)["q"].items()}
            res.append((f"{name}[{i + 1}]", slice(16 * i, 16 * i + 16), dict(cls, **_named({"pad": ~im, "image": im})), True))
        return res
    if name[0] == "X":
        bd = _border(H, W)
        return [(name, None, {"border": bd, "interior": ~bd}, True)]
    if name in ("t1act", "t1der", "t2act", "t2der", "srpre"):
        r = s if name == "srpre" else (4 if name[1] == "2" else (2 if s == 4 else s))
        bd = _border(H * r, W * r)
        cls = {"border": bd, "interior": ~bd}
        if name == "srpre":
            im = _inside(H * r, W * r, g.H0 * r, g.W0 * r)
            cls.update(_named({"crop": im, "outside": ~im}))
        return [(name, None, cls, True)]
    raise KeyError(name)


def required_entries(g):
    """The (entry, class) set a complete gate of this cell holds -- stated from the geometry, not read off ``errors``."""
    padded = g.H0 < g.H or g.W0 < g.W
    pad = ("pad", "image") if padded else ("image",)
    req = {("sr", "all")}

    def add(entry, classes):
        req.update((entry, c) for c in ("all", "chan_mean") + tuple(classes))

    add("X0", ("border", "interior") + pad)
    for b in range(g.nb):
        req.update({(f"b{b}.mean", "all"), (f"b{b}.rstd", "all")})
        for i in range(4):
            nh, nw = (g.H >> BR_L[i]) // 8, (g.W >> BR_L[i]) // 8
            kv = ("img_border", "cover1") + (("cover2",) if max(nh, nw) >= 2 else ()) + (("cover4",) if min(nh, nw) >= 2 else ())
            qc = ("win_corner",) + (("win_edge",) if max(nh, nw) >= 3 else ()) + (("win_interior",) if min(nh, nw) >= 3 else ())
            add(f"b{b}.d{i + 1}", kv + pad)
            if (i + 1) in g.stored_qkv:
                add(f"b{b}.qkv{i + 1}", kv + pad)
            add(f"b{b}.xc[{i + 1}]", qc + pad)
        add(f"X{b + 1}", ("border", "interior"))
    for n in ("t1act", "t1der") + (("t2act", "t2der") if g.scale == 4 else ()):
        add(n, ("border", "interior"))
    add("srpre", ("border", "interior", "crop") + (("outside",) if padded else ()))
    return req


def errors(g, got, ref):
    """{(entry, class): own-norm L2 error} over the stage outputs present in both."""
    e = {}
    for name in ref:
        if name not in got:
            continue
        for entry, sl, masks, cm in stage_classes(g, name):
            a, r = (got[name], ref[name]) if sl is None else (got[name][:, sl], ref[name][:, sl])
            a, r = a.detach().double(), r.detach().double()
            e[(entry, "all")] = A.own_norm_err(a, r)
            for cn, m in masks.items():
                e[(entry, cn)] = A.own_norm_err(a[..., m], r[..., m])
            if cm:
                rms = r.pow(2).mean(dim=(2, 3)).sqrt()
                e[(entry, "chan_mean")] = float((a.mean(dim=(2, 3)) - r.mean(dim=(2, 3))).norm() / (rms.norm() + 1e-300))
    return e


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
    """-> (failures, {(entry, class): (error, float32 oracle's error, ratio)}): <= 2e-5 of own norm, or <= 3 x the float32 oracle's error;
    sr: bit-equal."""
    table, bad = {}, []
    for k, e in err.items():
        o = o32.get(k, 0.0)
        table[k] = (e, o, e / o if o > 0 else (0.0 if e == 0 else math.inf))
        tol = 0.0 if k[0] == "sr" else FP32_TOL
        if not (e <= tol or e <= A.MARGIN * o):
            bad.append(f"{k[0]}[{k[1]}]: error {e:.3e} > {tol:g} and > {A.MARGIN:g} x the float32 oracle's {o:.3e}")
    return bad, table


def gate(g, taps):
    """The whole gate of one run's stage outputs `taps` (a device run's, or the emulation playing one) -> (failures, table, err)."""
    ref = reference(g, taps)
    err = errors(g, taps, ref)
    o32 = errors(g, oracle32(g, taps), ref)
    if g.dtype == "bf16":
        bad, table = gate_bf16(err, errors(g, emulate(g, taps), ref), floor=o32)
    else:
        bad, table = gate_fp32(err, o32)
    return bad, table, err


def format_table(table, third="ratio"):
    return "\n".join(f"    {t:10s} {c:12s} err {e:.3e}  ref {b:.3e}  {third} {q:6.2f}" for (t, c), (e, b, q) in table.items())
