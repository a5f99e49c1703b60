"""-m gpu: stage gate of the MedCLIP image tower (csrc/m2t_swin.hip): every kernel of the forward (both paths) and of the
backward against fp64, teacher-forced.

One handle per dtype (max_images 4); the cases of tests/swin_ref.py run on it in order, long ones first, so a short call
follows a long one on the same workspace; the `peaked` parameter set (swin_ref.PEAK) is loaded onto the same handle last.
Every reference is TEACHER-FORCED: the fp64 stage of tests/swin_ref.py applied to the DEVICE's own stage input, so an error is
charged to the stage that makes it.  Metric: the largest per-row relative L2 error over the token rows (`row_err`); for the
MLP half also the BRANCH metric (the same after subtracting the residual input from both sides).

  1. POISON.  Before every call the activation part of the workspace (everything behind the packed weights and fused biases),
     hidden_out, emb, grad_taps, g_crops and the grad workspace behind its transposed weights are filled with 0xFF bytes (NaN).
  2. DEFAULT PATH (m2t_swin_encode_ex, hidden_out): patch, embed_ln; per block qkv, attn_half, mlp_half and the whole block from
     its xin (the last block of a stage against m_s through the gather, the last of all against xf; the whole block is the check
     that found the text tower's layer 1: each stage inside its bound, the softmax amplifying the sum); merge x 3; final_ln; head; out of the workspace the
     last block's attention alone (AO), its fc1 + GELU (MH), and X / Hn / QKV bit-equal to xf / hnf / s3b1.qkv.  emb is
     bit-equal to the plain m2t_swin_encode / m2t_swin_encode_pair.
  3. GRAD PATH (m2t_swin_encode_grad, the stash through "gws:"): the same stages on the first n_grad crops, plus gder.
     fp32: emb and every stashed tensor bit-equal to the default path's.  bf16: bit-equal where both paths run the same
     kernels on the same bits: e0, s0b0.xin, s0b0.qkv, s0b0.xmid (from the first mlp_half on, the default path runs
     swin_mlp_fused_kernel at stages 0 / 1 and M2T_E_BIAS_GELU behind them, the grad path M2T_E_BIAS_SHUF with the fitted GELU,
     and the inputs of every later stage differ).
  4. BACKWARD (m2t_swin_backward_ex, grad_taps): every tap against the hand-written VJP of its stage (swin_ref, pinned to
     autograd by tests/test_swin_ref_cpu.py) at the device's stashed input with the device's previous tap as cotangent; the
     first against head_bwd + ln_bwd of g_emb, g_crops against embed_bwd of the last tap.  g_crops bit-equal to the plain call.
  5. OWNERSHIP.  Every byte outside the rows the call owns (n < 4, the tail of each region, MD behind n crops, the grad
     workspace behind the n_grad layout) still holds the fill; every owned element is finite.
  6. STALE BYTES.  The same call over another fill byte (0x5A): same bits in emb, hidden_out, the stash, the taps, g_crops.

BOUNDS.  fp32 forward: swin_ref.FP32_TOL = 2e-5 per stage.  bf16 forward: MARGIN = 3 x the error of the CPU emulation of that
stage against fp64 on the same input; emb (fp32, no bf16 store) takes the fp32 bound.  fp32 backward: the larger of FP32_TOL and
3 x the error of the same VJP in torch float32 on the CPU.  bf16 backward: MARGIN x the emulation's error; the two taps without
a bf16 store (the embedding LayerNorm's gF, g_crops) take the fp32 rule.  Branch metric of mlp_half: MARGIN x the error of the CPU
stand-in in that metric: the emulation (bf16), torch float32 (fp32) -- the larger of its two contraction orders, see FINDING.
Nothing is taken from the device.

FINDING of the first device run (no kernel fault; one bound restated).  Every stage, tap, ownership and bit-equality check of both
dtypes passed except the fp32 branch metric of mlp_half at stage 3: 1.03e-6 .. 1.23e-6 against 3 x torch float32's 2.4e-7 ..
3.3e-7 (every other block: at most 0.58 of its budget).  fc2 of stage 3 is the longest contraction of the tower (K = 3072), and the
fp32 BIAS_GELU / BIAS_RESID gemm_nt kernels sum it in ONE chain of 16x16x4 MFMA products per output, where the CPU BLAS behind
torch sums in blocks; a chain's rounding error grows with sqrt(K), a blocked sum's much slower.  Restated in the kernel's order
(swin_ref.Ref(chain=True): float32, one chain over K in steps of 4) the stand-in itself measures 5.9e-7 .. 6.2e-7 there (blocked:
3.7e-7 .. 4.3e-7; tests/test_swin_ref_cpu.py prints both), while at stages 0 - 2 the blocked order is the less accurate one.  Both
are correct float32 evaluations, so the budget is MARGIN x the LARGER of the two; the seeded gelu_tanh fault (5.4e-4) stays 70 x
above the largest such budget.

KERNEL -> STAGE.  swin_patchify_kernel, gemm_nt BIAS: patch | layernorm_kernel: embed_ln, qkv, mlp_half, merge, final_ln (C = 96,
192, 384, 768, 1536: every G / NV instantiation) | gemm_nt BIAS (qkv), BIAS_RESID (attn_half, mlp_half), BIAS_GELU (mlp_half
default path; mlp_hidden), BIAS_SHUF (gder, mlp_half grad path), PLAIN (merge; backward), GELU_GRAD (mlp_half_bwd) |
swin_attn_kernel: attn_half at shift 0 and shift 3 in stages 0, 1, 2 and shift 0 in stage 3; attn | swin_mlp_fused_kernel<96>:
mlp_half s0b0 / s0b1 bf16 default path (3136 n rows, whole tiles); swin_mlp_fused_kernel<192>: mlp_half s1b0 / s1b1 bf16 default
path with a ragged last tile of 16 rows (`one`) and 48 rows (`three`, `pair_edge`) | swin_merge_gather_kernel: mlp_half of the
last block of stages 0 - 2 (through the gather) | swin_head_kernel: head | swin_head_bwd_kernel, layernorm_bwd_kernel: tap xf |
gemm_nt GELU_GRAD / PLAIN, layernorm_bwd_kernel: taps *.xmid | swin_attn_bwd_kernel (shift 0 and 3 as above), gemm_nt PLAIN,
layernorm_bwd_kernel: taps *.xin | swin_merge_scatter_kernel: taps s*.out | layernorm_bwd_kernel (fp32 gradient in): tap e0 |
swin_embed_bwd_kernel: g_crops | convert / frag16_pack / transpose_convert (weight packing): through every GEMM stage.

WHAT BF16 CANNOT SEE (tests/test_swin_ref_cpu.py prints the ratios).  Of the seeded faults of swin_ref.BUGS the bf16 legs see all
but one at >= 8 x their budget (attention faults 8 .. 60 x, in the metric of the half-block; mlp_tail 147 x; gemm_row, gder_sign
50 x): `gelu_tanh` moves the MLP half by 1.1e-4 (branch 5.5e-4) against a bf16 budget of 0.13, so only the fp32 legs carry the
choice of GELU, and they carry it safely only in the BRANCH metric (5.5e-4 against 5 x FP32_TOL = 1e-4; the stage metric is AT
1e-4) -- which is why mlp_half's branch metric is bounded.  merge_order and ln_bwd_mean sit in stages without a bf16 store.

MEASURED on MI355X (one run of the suite; worst over the legs; s<k> = worst over the blocks of stage k; fp32: error / bound,
bf16: error / budget at the worst ratio).  In bf16 the device sits ON the emulation (ratio 1 / 3 = equal errors).
  stage                      fp32                                               bf16
  patch                      2.4e-06 / 2e-5                                     3.4e-02 / 1.0e-01 = 0.33
  embed_ln | final_ln        1.8e-07 | 1.4e-07 / 2e-5                           2.1e-03 / 6.2e-03 | 1.7e-03 / 5.2e-03 = 0.33
  qkv        s0 s1 s2 s3     1.1e-06 1.4e-06 1.1e-06 4.8e-07 / 2e-5             1.1e-02 / 3.2e-02 .. 2.7e-02 / 8.2e-02 = 0.33
  attn_half  s0 s1 s2 s3     3.2e-06 3.6e-06 6.5e-07 1.3e-07 / 2e-5             1.2e-02 / 3.5e-02 .. 1.8e-03 / 5.5e-03 = 0.33
  mlp_half   s0 s1 s2 s3     8.9e-07 8.2e-07 7.7e-07 2.5e-07 / 2e-5             3.8e-03 / 1.1e-02 .. 2.9e-03 / 8.1e-03 = 0.35
  mlp_half branch s0..s3     4.6e-06 / 1.1e-05  1.3e-06 / 3.1e-06               3.1e-02 / 9.2e-02 .. 9.4e-03 / 2.7e-02 = 0.34
                             2.2e-06 / 3.8e-06  1.1e-06 / 1.7e-06 (0.43 .. 0.68)
  block      s0 s1 s2 s3     4.2e-06 3.9e-06 3.4e-06 2.9e-07 / 2e-5 (peaked)    4.3e-03 / 1.2e-02 = 0.36
  gder (grad path)           <= 4.3e-07 / 2e-5                                  4.6e-03 / 1.4e-02 = 0.34
  merge                      3.8e-06 / 2e-5                                     2.0e-03 / 6.0e-03 = 0.33
  s3b1 attn | mlp_hidden     1.6e-07 | 6.9e-07 / 2e-5                           1.9e-03 / 5.5e-03 | 6.9e-03 / 2.1e-02 = 0.33
  head                       5.7e-07 / 2e-5                                     5.1e-07 / 2e-5
  tap xf                     2.8e-06 / 2e-5                                     1.6e-03 / 4.7e-03 = 0.33
  taps *.xmid                <= 3.0e-07 / 2e-5                                  2.4e-03 / 7.1e-03 = 0.33
  taps *.xin s3 s2 s1 s0     5.7e-06 6.5e-06 / 2e-5, 9.0e-04 / 2.6e-03          9.1e-02 / 2.7e-01 = 0.33
                             (peaked; torch float32 itself 8.7e-04), 6.2e-06 / 2e-5
  taps s*.out (scatter)      7.7e-06 / 2.5e-05                                  6.8e-02 / 2.0e-01 = 0.33
  tap e0 | g_crops           2.4e-07 | 3.8e-07 / 2e-5                           2.9e-07 | 3.1e-07 / 2e-5
DESIGN.md ("Swin stage gate") has the same table with the cases.
"""
import ctypes as C
import math

import pytest
import torch

from tests import swin_ref as R

pytestmark = pytest.mark.gpu

ACT = ("crops", "A0", "X", "Hn", "QKV", "AO", "MH", "emb")
GUARD = 4096


@pytest.fixture(scope="module")
def params():
    return {k: R.make_params(k) for k in ("closed", "peaked")}


@pytest.fixture(scope="module")
def encoders(params):
    made, loaded = {}, {}

    def get(dtype, kind):
        from m2trans_amd import _lib
        from m2trans_amd.losses import SwinEncoder
        if dtype not in made:
            made[dtype] = SwinEncoder(4, _lib.F32 if dtype == "fp32" else _lib.BF16, torch.device("cuda"))
            made[dtype].grad_workspace = torch.empty(int(_lib.load().m2t_swin_grad_workspace_bytes(made[dtype].handle, 2)),
                                                     dtype=torch.uint8, device="cuda")
        if loaded.get(dtype) != kind:
            made[dtype].load(params[kind])
            loaded[dtype] = kind
        return made[dtype]
    return get


def _crop_array(crops):
    return (C.c_int * (3 * len(crops)))(*[int(v) for c in crops for v in c])


def _views(buf, layout, tdt, es):
    """{name: tensor [n, rows, width]} of a byte buffer (CPU) by an element layout"""
    return {k: buf[o * es:(o + math.prod(shp)) * es].view(tdt).reshape(shp) for k, o, shp in layout}


class Run:
    """one call on poisoned buffers.  grad = None: m2t_swin_encode_ex; grad = n_grad: m2t_swin_encode_grad + m2t_swin_backward_ex"""

    def __init__(self, enc, dtype, name, fill, grad=None):
        from m2trans_amd import _lib
        from m2trans_amd.losses import SwinEncoder
        lib = _lib.load()
        self.tdt, self.es = (torch.float32, 4) if dtype == "fp32" else (torch.bfloat16, 2)
        self.dtype, self.grad, self.fill = dtype, grad, fill
        a, b, crops = R.case(name)
        self.n = n = len(crops)
        self.off = {k: enc.query("ws:" + k) for k in ACT}
        self.cnt = {k: enc.query("wsn:" + k) for k in ACT}
        self.esz = {k: (4 if k in ("crops", "emb") else self.es) for k in ACT}
        self.start = self.off["crops"]
        # the activation regions lie behind the packed weights and the fused biases, which must survive the fill
        assert enc.query("ws:packed") + enc.query("wsn:packed") * self.es <= enc.query("ws:fbias")
        assert enc.query("ws:fbias") + enc.query("wsn:fbias") * 4 <= self.start == min(self.off.values())
        enc.workspace[self.start:].fill_(fill)
        ad, bd = a.cuda(), (None if b is None else b.cuda())
        emb = torch.full((n * 512 * 4 + GUARD,), fill, dtype=torch.uint8, device="cuda")
        args = (enc.handle, _lib.ptr(ad), a.shape[0], _lib.ptr(bd), 0 if b is None else b.shape[0], a.shape[2], a.shape[3], _crop_array(crops), n)
        if grad is None:
            self.hlay = SwinEncoder.hidden_layout(n)
            self.hbytes = (self.hlay[-1][1] + math.prod(self.hlay[-1][2])) * self.es
            hidden = torch.full((self.hbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
            _lib.check(lib.m2t_swin_encode_ex(*args, _lib.ptr(emb), _lib.ptr(enc.workspace), _lib.stream_ptr(), _lib.ptr(hidden)),
                       "m2t_swin_encode_ex")
            torch.cuda.synchronize()
            self.hidden = hidden.cpu()
            self.hs = _views(self.hidden, self.hlay, self.tdt, self.es)
        else:
            ng = grad
            gws = enc.grad_workspace
            self.gbytes = int(lib.m2t_swin_grad_workspace_bytes(enc.handle, ng))          # the layout the gws: keys answer in
            assert self.gbytes <= gws.numel()
            self.gstart = enc.query("gws:gR")                                              # behind the transposed weights
            gws[self.gstart:].fill_(fill)
            self.tlay = SwinEncoder.tap_layout(ng)
            self.tbytes = (self.tlay[-1][1] + math.prod(self.tlay[-1][2])) * 4
            taps = torch.full((self.tbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
            gcr = torch.full((ng * 3 * 224 * 224 * 4 + GUARD,), fill, dtype=torch.uint8, device="cuda")
            gcr2 = torch.empty(ng * 3 * 224 * 224, dtype=torch.float32, device="cuda")
            self.g_emb = torch.sin(torch.arange(ng * 512, dtype=torch.float64) * 0.731 + 0.3).reshape(ng, 512).float()
            ge = self.g_emb.cuda()
            _lib.check(lib.m2t_swin_encode_grad(*args, ng, _lib.ptr(emb), _lib.ptr(enc.workspace), _lib.ptr(gws), _lib.stream_ptr()),
                       "m2t_swin_encode_grad")
            _lib.check(lib.m2t_swin_backward_ex(enc.handle, _lib.ptr(ge), ng, _lib.ptr(gcr), _lib.ptr(enc.workspace), _lib.ptr(gws),
                                                _lib.stream_ptr(), _lib.ptr(taps)), "m2t_swin_backward_ex")
            torch.cuda.synchronize()
            self.gws = gws[self.gstart:].cpu()
            self.taps_raw, self.gcr_raw = taps.cpu(), gcr.cpu()
            _lib.check(lib.m2t_swin_backward(enc.handle, _lib.ptr(ge), ng, _lib.ptr(gcr2), _lib.ptr(enc.workspace), _lib.ptr(gws),
                                             _lib.stream_ptr()), "m2t_swin_backward")
            torch.cuda.synchronize()
            self.g_crops_plain = gcr2.cpu().reshape(ng, 3, 224, 224)
            self.g_crops = self.gcr_raw[:ng * 3 * 224 * 224 * 4].view(torch.float32).reshape(ng, 3, 224, 224)
            self.taps = _views(self.taps_raw, self.tlay, torch.float32, 4)
            # the stash: name -> (byte offset behind gstart, owned elements, element size)
            self.greg = {}
            for k, _, shp in SwinEncoder.hidden_layout(ng):
                self.greg[k] = (enc.query("gws:" + k) - self.gstart, math.prod(shp), self.es, shp)
            for s, j in R.BLOCKS:
                H, Cc = R.dims(s)
                k = f"s{s}b{j}.gder"
                self.greg[k] = (enc.query("gws:" + k) - self.gstart, ng * H * H * 4 * Cc, self.es, (ng, H * H, 4 * Cc))
            tok = ng * 3136 * 96
            for k, mult, es in (("gR", 1, 4), ("gF", 1, 4), ("gT", 1, self.es), ("gC", 1, self.es), ("gQ", 3, self.es), ("gA", 4, self.es)):
                self.greg[k] = (enc.query("gws:" + k) - self.gstart, tok * mult, es, None)
            self.greg["MD"] = (enc.query("gws:MD") - self.gstart, n * 3136 * 96 * 4, self.es, None)
            for k, (o, cnt, es, _) in self.greg.items():
                assert cnt <= enc.query("gwsn:" + k) and 0 <= o and o + cnt * es <= self.gbytes - self.gstart, k
            self.stash = {k: self.gws[o:o + cnt * es].view(self.tdt).reshape(shp) for k, (o, cnt, es, shp) in self.greg.items() if shp}
        self.ws = enc.workspace[self.start:].cpu()
        self.emb_raw = emb.cpu()
        self.emb = self.emb_raw[:n * 512 * 4].view(torch.float32).reshape(n, 512)

    def owned(self, k):
        """elements of workspace region k the call writes"""
        n = self.n
        fused = self.dtype == "bf16" and self.grad is None                 # stages 0 / 1 keep the hidden tensor in LDS
        return {"crops": 3 * n, "A0": n * 3136 * 48, "X": n * 3136 * 96, "Hn": n * 3136 * 96, "QKV": n * 3136 * 288, "AO": n * 3136 * 96,
                "MH": n * 196 * 1536 if fused else n * 3136 * 384, "emb": 0}[k]

    def region(self, k, rows, width):
        o = self.off[k] - self.start
        return self.ws[o:o + self.n * rows * width * self.es].view(self.tdt).reshape(self.n, rows, width)

    def problems(self):
        """what check 5 finds: bytes outside the owned rows that lost the fill, owned elements that are not finite"""
        bad = []
        keep = torch.ones(self.ws.numel(), dtype=torch.bool)
        for k in ACT:
            o, nb = self.off[k] - self.start, self.owned(k) * self.esz[k]
            assert self.owned(k) <= self.cnt[k]
            keep[o:o + nb] = False
            if k != "crops" and nb and not bool(torch.isfinite(self.ws[o:o + nb].view(torch.float32 if k == "emb" else self.tdt).float()).all()):
                bad.append(f"workspace {k}: not finite")
        spoiled = torch.nonzero(keep & (self.ws != self.fill)).flatten()
        if len(spoiled):
            at = int(spoiled[0]) + self.start
            bad.append("workspace byte %d (region %s)" % (at, max((k for k in ACT if self.off[k] <= at), key=lambda k: self.off[k])))
        if not bool((self.emb_raw[self.n * 512 * 4:] == self.fill).all()):
            bad.append("emb tail")
        if not bool(torch.isfinite(self.emb).all()):
            bad.append("emb: not finite")
        if self.grad is None:
            if not bool((self.hidden[self.hbytes:] == self.fill).all()):
                bad.append("hidden_out tail")
            bad += [f"hidden {k}: not finite" for k, v in self.hs.items() if not bool(torch.isfinite(v.float()).all())]
            return bad
        keep = torch.ones(self.gws.numel(), dtype=torch.bool)
        for k, (o, cnt, es, shp) in self.greg.items():
            keep[o:o + cnt * es] = False
            if not bool(torch.isfinite(self.gws[o:o + cnt * es].view(torch.float32 if es == 4 else torch.bfloat16).float()).all()):
                bad.append(f"grad workspace {k}: not finite")
        spoiled = torch.nonzero(keep & (self.gws != self.fill)).flatten()
        if len(spoiled):
            at = int(spoiled[0])
            bad.append("grad workspace byte %d behind gR (region %s)" % (at, max((k for k in self.greg if self.greg[k][0] <= at),
                                                                                 key=lambda k: self.greg[k][0])))
        if not bool((self.taps_raw[self.tbytes:] == self.fill).all()):
            bad.append("grad_taps tail")
        if not bool((self.gcr_raw[self.grad * 3 * 224 * 224 * 4:] == self.fill).all()):
            bad.append("g_crops tail")
        bad += [f"tap {k}: not finite" for k, v in self.taps.items() if not bool(torch.isfinite(v).all())]
        if not bool(torch.isfinite(self.g_crops).all()):
            bad.append("g_crops: not finite")
        return bad


class Table:
    """(stage, error, budget) rows of one leg"""

    def __init__(self, dtype, name, kind, p):
        self.dtype, self.tag, self.rows = dtype, f"{dtype} {kind} {name}", []
        self.r64, self.r32, self.emu = R.Ref(p), R.Ref(p, dt=torch.float32), R.Ref(p, emu=True)
        self.r32c = R.Ref(p, dt=torch.float32, chain=True)          # float32 with the GEMMs summed in the kernel's order

    def _err(self, got, want):
        return R.row_err(got, want) if bool(torch.isfinite(got.float()).all()) else float("inf")

    def fwd(self, tag, got, fn, fp32_out=False, resid=None, bound_branch=False):
        """forward stage fn(ref): fp32 FP32_TOL; bf16 MARGIN x the emulation's error (fp32-typed outputs: FP32_TOL)"""
        want = fn(self.r64)
        budget = R.FP32_TOL if (self.dtype == "fp32" or fp32_out) else R.MARGIN * R.row_err(fn(self.emu), want)
        self.rows.append((tag, self._err(got, want), budget))
        if resid is not None:
            err = R.branch_err(got, want, resid) if bool(torch.isfinite(got.float()).all()) else float("inf")
            budget = None
            if bound_branch:
                stand_ins = (self.r32, self.r32c) if self.dtype == "fp32" else (self.emu,)
                budget = R.MARGIN * max(R.branch_err(fn(r), want, resid) for r in stand_ins)
            self.rows.append((tag + " [branch]", err, budget))

    def bwd(self, tag, got, fn, rounds=True):
        """backward stage: fp32 (and taps without a bf16 store) max(FP32_TOL, 3 x torch float32's error); bf16 MARGIN x the emulation's"""
        want = fn(self.r64)
        if self.dtype == "bf16" and rounds:
            budget = R.MARGIN * R.row_err(fn(self.emu), want)
        else:
            budget = max(R.FP32_TOL, 3.0 * R.row_err(fn(self.r32), want))
        self.rows.append((tag, self._err(got, want), budget))

    def over(self):
        for tag, err, budget in self.rows:
            print(f"{self.tag:22s} {tag:24s} err {err:.3e} " + ("(reported)" if budget is None else f"budget {budget:.3e}")
                  + ("" if budget is None or err <= budget else "   <-- OVER"))
        return [(t, e, b) for t, e, b in self.rows if b is not None and not e <= b]


def _forward_stages(t, hs, crops, grad):
    """checks 2 / 3: the stage chain on the tensors hs of one path (hidden_out, or the stash of the first n_grad crops)"""
    t.fwd("patch", hs["e0"], lambda r: r.patch(crops))
    t.fwd("embed_ln", hs["s0b0.xin"], lambda r: r.embed_ln(hs["e0"]))
    for s in range(4):
        for j in range(R.DEPTHS[s]):
            k = f"s{s}b{j}."
            xin, qkv, xmid = hs[k + "xin"], hs[k + "qkv"], hs[k + "xmid"]
            t.fwd(k + "qkv", qkv, lambda r: r.qkv(xin, s, j))
            t.fwd(k + "attn_half", xmid, lambda r: r.attn_half(qkv, xin, s, j), resid=xin)
            if j + 1 < R.DEPTHS[s]:
                t.fwd(k + "mlp_half", hs[f"s{s}b{j + 1}.xin"], lambda r: r.mlp_half(xmid, s, j), resid=xmid, bound_branch=True)
                t.fwd(k + "block", hs[f"s{s}b{j + 1}.xin"], lambda r: r.block(xin, s, j))
            elif s < 3:
                t.fwd(k + "mlp_half", hs[f"m{s}"], lambda r: r.gather(r.mlp_half(xmid, s, j)), resid=R.gather_perm(xmid), bound_branch=True)
                t.fwd(k + "block", hs[f"m{s}"], lambda r: r.gather(r.block(xin, s, j)))
            else:
                t.fwd(k + "mlp_half", hs["xf"], lambda r: r.mlp_half(xmid, s, j), resid=xmid, bound_branch=True)
                t.fwd(k + "block", hs["xf"], lambda r: r.block(xin, s, j))
            if grad:
                t.fwd(k + "gder", hs[k + "gder"], lambda r: r.gder(xmid, s, j))
        if s < 3:
            t.fwd(f"merge{s}", hs[f"s{s + 1}b0.xin"], lambda r: r.merge(hs[f"m{s}"], s))
    t.fwd("final_ln", hs["hnf"], lambda r: r.final_ln(hs["xf"]))


def _param_ids():
    legs = [("fp32", c, "closed") for c in R.CASES] + [("fp32", "three", "peaked")]
    legs += [("bf16", c, "closed") for c in R.BF16_CASES] + [("bf16", "three", "peaked")]
    return legs


LEGS = _param_ids()
GRAD_LEGS = [(d, c, k) for d, c, k in LEGS if c in R.GRAD_CASES]
_RUNS = {}                                      # (dtype, case, kind) -> default-path Run, for the grad test of the same leg


def _plain_emb(enc, name):
    a, b, crops = R.case(name)
    return (enc.encode(a.cuda(), crops) if b is None else enc.encode_pair(a.cuda(), b.cuda(), crops)).cpu()


@pytest.mark.parametrize("dtype,name,kind", LEGS, ids=[f"{d}-{c}-{k}" for d, c, k in LEGS])
def test_swin_default_path_stages_against_fp64(dtype, name, kind, params, encoders):
    """checks 1, 2, 5, 6 of the module docstring"""
    enc = encoders(dtype, kind)
    run = _RUNS[dtype, name, kind] = Run(enc, dtype, name, 0xFF)
    t, hs, crops = Table(dtype, name, kind, params[kind]), run.hs, R.crops_of(name)
    bad = run.problems()
    _forward_stages(t, hs, crops, False)
    t.fwd("head", run.emb, lambda r: r.head(hs["hnf"]), fp32_out=True)
    # the last block out of the workspace: the attention kernel and fc1 + GELU on their own
    t.fwd("s3b1.attn", run.region("AO", 49, 768), lambda r: r.attn(hs["s3b1.qkv"], 3, 1))
    t.fwd("s3b1.mlp_hidden", run.region("MH", 49, 3072), lambda r: r.mlp_hidden(hs["s3b1.xmid"], 3, 1))
    over = t.over()
    norm_off = float((run.emb.norm(dim=1) - 1).abs().max())
    again = Run(enc, dtype, name, 0x5A)
    plain = _plain_emb(enc, name)
    assert not bad, bad
    assert not again.problems()
    assert not over, over
    bits = lambda v: v.contiguous().view(torch.uint8)
    assert torch.equal(bits(run.region("X", 49, 768)), bits(hs["xf"])) and torch.equal(bits(run.region("Hn", 49, 768)), bits(hs["hnf"]))
    assert torch.equal(bits(run.region("QKV", 49, 2304)), bits(hs["s3b1.qkv"]))
    assert norm_off < 1e-4, norm_off
    assert torch.equal(plain, run.emb), "m2t_swin_encode_ex changes emb"
    assert torch.equal(again.emb.view(torch.int32), run.emb.view(torch.int32)), "emb depends on stale workspace bytes"
    assert torch.equal(again.hidden[:run.hbytes], run.hidden[:run.hbytes]), "hidden states depend on stale workspace bytes"


@pytest.mark.parametrize("dtype,name,kind", GRAD_LEGS, ids=[f"{d}-{c}-{k}" for d, c, k in GRAD_LEGS])
def test_swin_grad_path_and_backward_against_fp64(dtype, name, kind, params, encoders):
    """checks 1, 3, 4, 5, 6 of the module docstring"""
    enc = encoders(dtype, kind)
    if (dtype, name, kind) not in _RUNS:
        _RUNS[dtype, name, kind] = Run(enc, dtype, name, 0xFF)
    ref, ng = _RUNS[dtype, name, kind], R.GRAD_CASES[name]
    run = Run(enc, dtype, name, 0xFF, grad=ng)
    t, hs, tp, crops = Table(dtype, name, kind, params[kind]), run.stash, run.taps, R.crops_of(name)[:ng]
    bad = run.problems()
    # 3. forward stages of the grad path on the stash
    _forward_stages(t, hs, crops, True)
    t.fwd("head", run.emb[:ng], lambda r: r.head(hs["hnf"]), fp32_out=True)
    # 4. the taps, in backward order
    t.bwd("tap xf", tp["xf"], lambda r: r.ln_bwd(hs["xf"], r.head_bwd(hs["hnf"], run.g_emb), "layernorm.weight"))
    prev = tp["xf"]
    for s in (3, 2, 1, 0):
        for j in reversed(range(R.DEPTHS[s])):
            k = f"s{s}b{j}."
            t.bwd("tap " + k + "xmid", tp[k + "xmid"], lambda r: r.mlp_half_bwd(hs[k + "xmid"], hs[k + "gder"], prev, s, j))
            prev = tp[k + "xmid"]
            t.bwd("tap " + k + "xin", tp[k + "xin"], lambda r: r.attn_half_bwd(hs[k + "xin"], hs[k + "qkv"], prev, s, j))
            prev = tp[k + "xin"]
        if s > 0:
            t.bwd(f"tap s{s - 1}.out", tp[f"s{s - 1}.out"], lambda r: r.merge_bwd(hs[f"m{s - 1}"], prev, s - 1))
            prev = tp[f"s{s - 1}.out"]
    t.bwd("tap e0", tp["e0"], lambda r: r.embed_ln_bwd(hs["e0"], prev), rounds=False)
    t.bwd("g_crops", run.g_crops.reshape(ng, 3 * 224, 224), lambda r: r.embed_bwd(tp["e0"]).reshape(ng, 3 * 224, 224), rounds=False)
    over = t.over()
    again = Run(enc, dtype, name, 0x5A, grad=ng)
    assert not bad, bad
    assert not again.problems()
    assert not over, over
    assert float((run.emb.norm(dim=1) - 1).abs().max()) < 1e-4
    bits = lambda v: v.contiguous().view(torch.uint8)
    assert torch.equal(run.g_crops_plain, run.g_crops), "m2t_swin_backward_ex changes g_crops"
    same = list(ref.hs) if dtype == "fp32" else ["e0", "s0b0.xin", "s0b0.qkv", "s0b0.xmid"]
    diff = [k for k in same if not torch.equal(bits(ref.hs[k][:ng]), bits(hs[k]))]
    assert not diff, diff
    if dtype == "fp32":
        assert torch.equal(ref.emb, run.emb), "the grad path's emb is not the default path's"
    assert torch.equal(again.emb.view(torch.int32), run.emb.view(torch.int32)), "emb depends on stale bytes"
    assert torch.equal(again.taps_raw[:run.tbytes], run.taps_raw[:run.tbytes]), "the taps depend on stale bytes"
    assert torch.equal(again.g_crops, run.g_crops), "g_crops depends on stale bytes"
    for k, (o, cnt, es, shp) in run.greg.items():
        if shp:
            assert torch.equal(again.gws[o:o + cnt * es], run.gws[o:o + cnt * es]), f"stash {k} depends on stale bytes"


def test_encoder_wrappers_are_the_plain_calls(params, encoders):
    """SwinEncoder.encode(..., hidden_states=True) and .backward(..., taps=True): the plain calls' bits, documented shapes"""
    enc = encoders("fp32", "peaked")
    a, b, crops = R.case("one")
    emb = enc.encode(a.cuda(), crops)
    emb2, hs = enc.encode(a.cuda(), crops, hidden_states=True)
    assert torch.equal(emb, emb2) and hs["s2b5.qkv"].shape == (1, 196, 1152) and hs["m0"].shape == (1, 784, 384) and hs["e0"].dtype == torch.float32
    assert R.row_err(hs["e0"].cpu(), R.Ref(params["peaked"]).patch(R.crops_of("one"))) < R.FP32_TOL
    enc.encode_grad(a.cuda(), None, crops, 1)
    g = torch.ones(1, 512, device="cuda")
    g1 = enc.backward(g, 1)
    g2, taps = enc.backward(g, 1, taps=True)
    assert torch.equal(g1, g2) and taps["xf"].shape == (1, 49, 768) and taps["s0.out"].shape == (1, 3136, 96) and len(taps) == 29


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_backward_after_a_relayout_of_the_grad_workspace(dtype, params):
    """m2t_swin_grad_workspace_bytes(h, 2) between encode_grad(n_grad = 1) and backward(n_grad = 1) re-lays the cached region table;
    backward lays it for its own n_grad again, so g_crops, emb and gws:gR are those of the undisturbed sequence, bit for bit"""
    from m2trans_amd import _lib
    from m2trans_amd.losses import SwinEncoder
    lib = _lib.load()
    enc = SwinEncoder(2, _lib.F32 if dtype == "fp32" else _lib.BF16, torch.device("cuda"))
    enc.grad_workspace = torch.empty(int(lib.m2t_swin_grad_workspace_bytes(enc.handle, 2)), dtype=torch.uint8, device="cuda")
    enc.load(params["closed"])
    src = torch.rand(1, 3, 240, 256, generator=torch.Generator().manual_seed(5)).cuda()
    crops, g_emb = [(0, 0, 0), (0, 16, 32)], torch.randn(1, 512, generator=torch.Generator().manual_seed(6)).cuda()
    emb_a = enc.encode_grad(src, None, crops, 1)
    g_a, gr_a = enc.backward(g_emb, 1), enc.query("gws:gR")
    emb_b = enc.encode_grad(src, None, crops, 1)
    assert lib.m2t_swin_grad_workspace_bytes(enc.handle, 2) == enc.grad_workspace.numel() and enc.query("gwsn:gR") == 2 * 3136 * 96
    g_b = enc.backward(g_emb, 1)
    assert enc.query("gws:gR") == gr_a and enc.query("gwsn:gR") == 3136 * 96
    assert torch.isfinite(g_a).all() and float(g_a.abs().max()) > 0
    assert torch.equal(emb_a.view(torch.int32), emb_b.view(torch.int32))
    assert torch.equal(g_a.view(torch.int32), g_b.view(torch.int32))
