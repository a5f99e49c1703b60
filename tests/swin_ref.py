"""Stage-level gate of the MedCLIP image tower (csrc/m2t_swin.hip, k_swin.hip, k_swin_bwd.hip): fp64 restatement per stage,
bf16 emulation, hand-written VJPs, metric, cases, seeded faults.

Plain helper module (CPU only, no pytest hooks), shared by tests/test_swin_ref_cpu.py and tests/test_gpu_swin_stages.py.
Weights: oracle.swin_oracle.closed_form_swin_params (``make_params``), and a PEAKED variant of them (``PEAK`` below).

Every tensor is [n][T][C]: n crops, T = H x H token rows in image order (row-major), C channels.  Stage s has H = 56 / 2^s,
C = 96 . 2^s, HEADS[s] heads of 32, DEPTHS[s] blocks; block j is shifted by 3 when j is odd and H > 7.

FORWARD STAGES of ``Ref`` (input -> output; the names are those of SwinEncoder.hidden_layout / "gws:"):
  patch         crop [n,3,224,224] -> e0        patchify (rounds the pixels), GEMM + bias         swin_patchify, gemm_nt BIAS
  embed_ln      e0 -> s0b0.xin                  LayerNorm                                          layernorm_kernel
  qkv           xin -> qkv                      LayerNorm, GEMM + bias                             layernorm_kernel, gemm_nt BIAS
  attn          qkv -> AO                       (shifted) window attention                         swin_attn_kernel
  attn_half     (qkv, xin) -> xmid              attn, o_proj + bias + residual                     + gemm_nt BIAS_RESID
  mlp_hidden    xmid -> MH                      LayerNorm, fc1 + bias + erf GELU                   layernorm_kernel, gemm_nt BIAS_GELU
  mlp_half      xmid -> next xin | m_s | xf     + fc2 + bias + residual                            + gemm_nt BIAS_RESID, or
                                                                                                   swin_mlp_fused_kernel (all of it)
  gder          xmid -> gelu'(fc1(LN(xmid)))    grad mode only                                     gemm_nt BIAS_SHUF
  gather        x -> m_s                        2 x 2 gather, a permutation                        swin_merge_gather_kernel
  merge         m_s -> s{s+1}b0.xin             LayerNorm(4C), reduction GEMM                      layernorm_kernel, gemm_nt PLAIN
  final_ln      xf -> hnf                       LayerNorm
  head          hnf -> emb (fp32)               token mean, Linear(768, 512), L2 normalise         swin_head_kernel

BACKWARD STAGES (hand-written VJPs; g* are the device's names):
  head_bwd      (hnf, g_emb) -> gC              stored in the compute type                         swin_head_bwd_kernel
  ln_bwd        (x, g, gamma) -> dx             LayerNorm VJP, fp32 out                            layernorm_bwd_kernel
  mlp_half_bwd  (xmid, gder, gR) -> gR'         gT = st(gR); gA = st(gT W2 o gder); gC = st(gA W1); ln_bwd + gR
  attn_half_bwd (xin, qkv, gR) -> gR'           gT; gC = st(gT Wo); gQ = st(attention VJP); gC = st(gQ Wqkv); ln_bwd + gR
  merge_bwd     (m_s, gR) -> gR'                gT; gC = st(gT Wred); gF = ln_bwd (fp32); scatter  swin_merge_scatter_kernel
  embed_ln_bwd  (e0, gR) -> gF                  ln_bwd on the fp32 gradient
  embed_bwd     gF -> g_crops                   projection^T + patchify adjoint, fp32              swin_embed_bwd_kernel

BF16 EMULATION (``emu=True``).  The rounding points are read off the code, not off a run.  Stored as bf16: the patchified
pixels (A0), every packed / transposed GEMM weight, every LayerNorm output (Hn; in the fused MLP the LDS copy), e0, xin, xmid,
qkv, AO, MH (in the fused MLP the LDS copy), gder, m_s, hnf; in swin_attn_kernel the PROBABILITIES are rounded before P.V;
backward: gT, gC, gQ, gA (swin_attn_bwd_kernel itself keeps everything fp32 in LDS).  Read as fp32: biases, LayerNorm
parameters, the relative-position tables, the projection head, the residual-stream gradient gR / gF, g_emb, g_crops.  Every GEMM,
LayerNorm and softmax accumulates in fp32 and rounds once, at its store; that accumulation is not emulated (1e-7, three orders
below a bf16 store).  ``emu=False`` is the plain stage in ``dt`` (float64: the reference; float32: the CPU stand-in for the
error an fp32 kernel may make).

METRIC.  ``row_err`` of tests/text_ref.py: the largest per-row relative L2 error over the token rows.  For the two residual
half-blocks also the BRANCH metric ``branch_err``: the same after subtracting the stage's own residual input from both sides, so
a fault in the branch is not diluted by the residual.

``BUGS`` are emulated kernel faults for the discrimination test of tests/test_swin_ref_cpu.py.
"""
from __future__ import annotations

import math

import torch

from oracle import swin_oracle as S
from tests.text_ref import FP32_TOL, MARGIN, row_err  # noqa: F401  (the project's per-stage bounds and metric)

DEPTHS, HEADS, EPS = S.DEPTHS, S.HEADS, S.LN_EPS
BLOCKS = [(s, j) for s in range(4) for j in range(DEPTHS[s])]
# the `peaked` set: the query and key weights and biases of stage s times PEAK[s].  One factor per stage, because the
# closed-form set is already selective at stage 0 (median largest probability per query 0.76: |q|, |k| reach 7.8) and nearly
# uniform behind it (0.04 .. 0.07 against 1 / 49 = 0.02): a single factor is held to 1.5 by stage 0 and leaves the other ten
# blocks uniform.  Each PEAK[s] is the largest of PEAK_CANDIDATES for which torch float32 against fp64, block by block and
# teacher-forced on `three`, stays within FP32_TOL / 4 on every block of the stage, stages chosen in order (measured:
# stage 0  1.5 -> 4.1e-6, 2 -> 6.1e-6;  stage 1  24 -> 4.4e-6, 32 -> 5.4e-6;  stage 2  16 -> 4.1e-6, 24 -> 5.6e-6;
# stage 3  32 -> 1.0e-7, the end of the list).  Median largest probability per query with them: 0.97, 0.99, 0.88, 0.53.
PEAK = (1.5, 24.0, 16.0, 32.0)
PEAK_CANDIDATES = (1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 24.0, 32.0)
BUGS = ("last_key", "mask_frame", "mask_off", "rel_swap", "no_rollback", "mlp_tail", "merge_order", "gemm_row", "gelu_tanh",
        "gder_sign", "ln_bwd_mean")
BUG_STAGE = {"last_key": "attn_half", "mask_frame": "attn_half", "mask_off": "attn_half", "rel_swap": "attn_half",
             "no_rollback": "attn_half", "mlp_tail": "mlp_half", "merge_order": "gather", "gemm_row": "qkv", "gelu_tanh": "mlp_half",
             "gder_sign": "gder", "ln_bwd_mean": "ln_bwd"}


def dims(s):
    """stage s -> (H, C)"""
    return 56 >> s, 96 << s


def shift_of(s, j):
    return 3 if (j % 2 == 1 and dims(s)[0] > 7) else 0


def make_params(kind="closed"):
    """fp32 parameters by HF name: the closed-form set, or `peaked`: its query / key weights and biases of stage s times PEAK[s]"""
    p = S.closed_form_swin_params()
    if kind == "peaked":
        return peaked(p, PEAK)
    assert kind == "closed"
    return p


def peaked(p, factors):
    """query / key weights and biases of stage s times factors[s]"""
    def f(k):
        return factors[int(k.split(".")[2])] if (".attention.self.query." in k or ".attention.self.key." in k) else 1.0
    return {k: v * f(k) for k, v in p.items()}


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def branch_err(got, want, resid) -> float:
    r = resid.to(torch.float64)
    return row_err(got.to(torch.float64) - r, want.to(torch.float64) - r)


def layer_norm(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * g + b


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf_grad(x, sign=1.0):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + sign * x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def to_windows(x, shift):
    """[n, H, H, ...] image order -> [n, nW, 49, ...] in the frame rolled by -shift"""
    n, H = x.shape[0], x.shape[1]
    rest = x.shape[3:]
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    nw = H // 7
    x = x.reshape(n, nw, 7, nw, 7, *rest).transpose(2, 3)
    return x.reshape(n, nw * nw, 49, *rest)


def from_windows(x, shift, rollback=True):
    """inverse of to_windows: [n, nW, 49, ...] -> [n, H, H, ...]"""
    n, nW = x.shape[0], x.shape[1]
    rest = x.shape[3:]
    nw = math.isqrt(nW)
    x = x.reshape(n, nw, nw, 7, 7, *rest).transpose(2, 3).reshape(n, nw * 7, nw * 7, *rest)
    if shift and rollback:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x


def region_ids(H, shift, frame_bug=False):
    """[H, H] region id of the shift mask, a function of the position in the ROLLED frame"""
    r = (torch.arange(H) >= H - 7).long() + (torch.arange(H) >= H - shift).long()
    ids = r[:, None] * 3 + r[None, :]
    if frame_bug:                          # evaluated at the un-rolled coordinate of the token instead
        ids = torch.roll(ids, shifts=(-shift, -shift), dims=(0, 1))
    return ids


def window_mask(H, shift, bugs=()):
    """[nW, 49, 49] additive mask: -100 between tokens of different regions"""
    ids = to_windows(region_ids(H, shift, "mask_frame" in bugs)[None], 0)[0]          # [nW, 49]
    m = (ids[:, :, None] != ids[:, None, :]).to(torch.float64) * -100.0
    if "mask_off" in bugs:
        nw = H // 7
        w = torch.arange(nw * nw)
        m[(w // nw == nw - 1) | (w % nw == nw - 1)] = 0.0
    return m


def rel_index(swap=False):
    co = torch.stack(torch.meshgrid(torch.arange(7), torch.arange(7), indexing="ij")).flatten(1)
    rel = co[:, :, None] - co[:, None, :]
    dh, dw = (rel[1], rel[0]) if swap else (rel[0], rel[1])
    return (dh + 6) * 13 + (dw + 6)


def gather_perm(x, bugs=()):
    """[n, H*H, C] -> [n, H*H/4, 4C], concat order (r0,c0),(r1,c0),(r0,c1),(r1,c1)  (swin_merge_gather_kernel)"""
    n, T, C = x.shape
    H = math.isqrt(T)
    x = x.reshape(n, H, H, C)
    order = [(0, 0), (0, 1), (1, 0), (1, 1)] if "merge_order" in bugs else [(0, 0), (1, 0), (0, 1), (1, 1)]
    return torch.cat([x[:, r::2, c::2, :] for r, c in order], dim=-1).reshape(n, T // 4, 4 * C)


def scatter_perm(y):
    """inverse (and adjoint) of gather_perm: [n, T/4, 4C] -> [n, T, C]"""
    n, T4, C4 = y.shape
    h, C = math.isqrt(T4), C4 // 4
    x = y.new_empty(n, 2 * h, 2 * h, C)
    y = y.reshape(n, h, h, 4, C)
    for part, (r, c) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        x[:, r::2, c::2, :] = y[:, :, :, part, :]
    return x.reshape(n, 4 * T4, C)


class Ref:
    """the stages on parameters p: emu=False in dtype dt (float64 reference / float32 stand-in), emu=True with the bf16 stores"""

    def __init__(self, p, emu=False, dt=torch.float64, bugs=(), chain=False):
        self.p, self.emu, self.dt, self.bugs, self.chain = p, emu, dt, tuple(bugs), chain

    # ---- helpers ----
    def f(self, name):
        return self.p[name].to(self.dt)

    def w(self, name):
        return self.st(self.f(name))

    def st(self, t):
        return bf16(t) if self.emu else t

    def x(self, t):
        return t.to(self.dt)

    def mm(self, x, w):
        """x [..., K] times w [N, K]^T.  chain=True (with dt = float32): ONE accumulation chain over K in steps of 4, the order of the
        fp32 gemm_nt epilogue kernels (a chain of 16x16x4 MFMA products per output) instead of the blocked sums of a CPU BLAS"""
        if not self.chain:
            return x @ w.T
        acc = torch.zeros(*x.shape[:-1], w.shape[0], dtype=self.dt)
        for k in range(0, x.shape[-1], 4):
            acc = acc + x[..., k:k + 4] @ w[:, k:k + 4].T
        return acc

    @staticmethod
    def blk(s, j):
        return f"encoder.layers.{s}.blocks.{j}."

    def ln(self, x, pre):
        return self.st(layer_norm(self.x(x), self.f(pre + ".weight"), self.f(pre + ".bias")))

    def wqkv(self, s, j):
        b = self.blk(s, j) + "attention.self."
        return torch.cat([self.w(b + nm + ".weight") for nm in ("query", "key", "value")]), \
            torch.cat([self.f(b + nm + ".bias") for nm in ("query", "key", "value")])

    # ---- forward ----
    def patch(self, crops):
        n = crops.shape[0]
        a0 = self.st(self.x(crops).reshape(n, 3, 56, 4, 56, 4).permute(0, 2, 4, 1, 3, 5).reshape(n, 3136, 48))
        w = self.w("embeddings.patch_embeddings.projection.weight").reshape(96, 48)
        return self.st(self.mm(a0, w) + self.f("embeddings.patch_embeddings.projection.bias"))

    def embed_ln(self, e0):
        return self.ln(e0, "embeddings.norm")

    def qkv(self, xin, s, j):
        w, b = self.wqkv(s, j)
        y = self.st(self.mm(self.ln(xin, self.blk(s, j) + "layernorm_before"), w) + b)
        if "gemm_row" in self.bugs:
            y = y.clone()
            y[-1, -1] = 0.0                                  # the last row never written (a zeroed buffer underneath)
        return y

    def _scores(self, q, k, s, j):
        """q, k [n, nW, heads, 49, 32] -> scores with table and mask"""
        H, shift = dims(s)[0], shift_of(s, j)
        tab = self.f(self.blk(s, j) + "attention.self.relative_position_bias_table")
        bias = tab[rel_index("rel_swap" in self.bugs).reshape(-1)].reshape(49, 49, HEADS[s]).permute(2, 0, 1)
        sc = q @ k.transpose(-1, -2) * (32 ** -0.5) + bias
        if shift:
            sc = sc + window_mask(H, shift, self.bugs).to(self.dt)[None, :, None]
        if "last_key" in self.bugs:
            sc = sc.clone()
            sc[..., 48] = -math.inf
        return sc

    def _split(self, qkv_t, s, j):
        n, T, C3 = qkv_t.shape
        H = math.isqrt(T)
        win = to_windows(self.x(qkv_t).reshape(n, H, H, 3, HEADS[s], 32), shift_of(s, j))    # [n, nW, 49, 3, heads, 32]
        win = win.permute(3, 0, 1, 4, 2, 5)                                                 # [3, n, nW, heads, 49, 32]
        return win[0], win[1], win[2]

    def attn(self, qkv_t, s, j):
        """qkv [n, T, 3C] -> AO [n, T, C]"""
        n, T, C3 = qkv_t.shape
        q, k, v = self._split(qkv_t, s, j)
        P = self.st(torch.softmax(self._scores(q, k, s, j), dim=-1))
        o = (P @ v).permute(0, 1, 3, 2, 4).reshape(n, -1, 49, C3 // 3)                       # [n, nW, 49, C]
        return self.st(from_windows(o, shift_of(s, j), "no_rollback" not in self.bugs).reshape(n, T, C3 // 3))

    def attn_half(self, qkv_t, xin, s, j):
        b = self.blk(s, j) + "attention.output.dense."
        return self.st(self.mm(self.attn(qkv_t, s, j), self.w(b + "weight")) + self.f(b + "bias") + self.x(xin))

    def _fc1_pre(self, xmid, s, j):
        b = self.blk(s, j)
        return self.mm(self.ln(xmid, b + "layernorm_after"), self.w(b + "intermediate.dense.weight")) + self.f(b + "intermediate.dense.bias")

    def mlp_hidden(self, xmid, s, j):
        t = self._fc1_pre(xmid, s, j)
        return self.st(gelu_tanh(t) if "gelu_tanh" in self.bugs else gelu_erf(t))

    def mlp_half(self, xmid, s, j):
        b = self.blk(s, j) + "output.dense."
        y = self.st(self.mm(self.mlp_hidden(xmid, s, j), self.w(b + "weight")) + self.f(b + "bias") + self.x(xmid))
        if "mlp_tail" in self.bugs:
            rows = y.reshape(-1, y.shape[-1])
            tail = rows.shape[0] % 64
            if tail:
                rows = rows.clone()
                rows[-tail:] = rows[-1]
                y = rows.reshape(y.shape)
        return y

    def gder(self, xmid, s, j):
        return self.st(gelu_erf_grad(self._fc1_pre(xmid, s, j), -1.0 if "gder_sign" in self.bugs else 1.0))

    def gather(self, x):
        return gather_perm(self.x(x), self.bugs)

    def merge(self, m, s):
        d = f"encoder.layers.{s}.downsample."
        return self.st(self.mm(self.ln(m, d + "norm"), self.w(d + "reduction.weight")))

    def final_ln(self, xf):
        return self.ln(xf, "layernorm")

    def head(self, hnf):
        e = self.x(hnf).mean(dim=1) @ self.f("projection_head.weight").T
        return e / e.norm(dim=-1, keepdim=True)

    def block(self, xin, s, j):
        return self.mlp_half(self.attn_half(self.qkv(xin, s, j), xin, s, j), s, j)

    def encode(self, crops):
        """-> (emb, {name: tensor}) with the names of SwinEncoder.hidden_layout"""
        hs = {"e0": self.patch(crops)}
        x = self.embed_ln(hs["e0"])
        for s in range(4):
            for j in range(DEPTHS[s]):
                k = f"s{s}b{j}."
                hs[k + "xin"] = x
                hs[k + "qkv"] = self.qkv(x, s, j)
                hs[k + "xmid"] = self.attn_half(hs[k + "qkv"], x, s, j)
                x = self.mlp_half(hs[k + "xmid"], s, j)
            if s < 3:
                hs[f"m{s}"] = self.gather(x)
                x = self.merge(hs[f"m{s}"], s)
        hs["xf"] = x
        hs["hnf"] = self.final_ln(x)
        return self.head(hs["hnf"]), hs

    # ---- backward (hand-written VJPs) ----
    def head_bwd(self, hnf, g_emb):
        """-> gradient w.r.t. hnf, stored in the compute type"""
        P = self.f("projection_head.weight")
        e = self.x(hnf).mean(dim=1) @ P.T
        nrm = e.norm(dim=-1, keepdim=True)
        u, g = e / nrm, self.x(g_emb)
        ge = (g - u * (u * g).sum(-1, keepdim=True)) / nrm
        return self.st(((ge @ P) / 49.0)[:, None, :].expand(-1, 49, -1))

    def ln_bwd(self, x, g, gamma_name, resid=None):
        x, gg = self.x(x), self.x(g) * self.f(gamma_name)
        mu = x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + EPS)
        xh = (x - mu) * rstd
        sg = 0.0 if "ln_bwd_mean" in self.bugs else gg.mean(-1, keepdim=True)
        d = rstd * (gg - sg - xh * (gg * xh).mean(-1, keepdim=True))
        return d if resid is None else d + self.x(resid)

    def mlp_half_bwd(self, xmid, gder, gR, s, j):
        b = self.blk(s, j)
        gT = self.st(self.x(gR))
        gA = self.st(gT @ self.w(b + "output.dense.weight") * self.x(gder))
        gC = self.st(gA @ self.w(b + "intermediate.dense.weight"))
        return self.ln_bwd(xmid, gC, b + "layernorm_after.weight", gR)

    def attn_bwd(self, qkv_t, gO, s, j):
        """VJP of `attn` without its stores (the kernel keeps everything fp32): (qkv, d AO) -> d qkv [n, T, 3C]"""
        n, T, C3 = qkv_t.shape
        H, C, shift = math.isqrt(T), C3 // 3, shift_of(s, j)
        q, k, v = self._split(qkv_t, s, j)
        dO = to_windows(self.x(gO).reshape(n, H, H, HEADS[s], 32), shift).permute(0, 1, 3, 2, 4)      # [n, nW, heads, 49, 32]
        P = torch.softmax(self._scores(q, k, s, j), dim=-1)
        dV = P.transpose(-1, -2) @ dO
        dP = dO @ v.transpose(-1, -2)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        dQ, dK = dS @ k * (32 ** -0.5), dS.transpose(-1, -2) @ q * (32 ** -0.5)
        g = torch.stack([dQ, dK, dV], dim=2).permute(0, 1, 4, 2, 3, 5).reshape(n, -1, 49, C3)         # [n, nW, 49, 3C]
        return from_windows(g, shift).reshape(n, T, C3)

    def attn_half_bwd(self, xin, qkv_t, gR, s, j):
        b = self.blk(s, j)
        gT = self.st(self.x(gR))
        gC = self.st(gT @ self.w(b + "attention.output.dense.weight"))
        gQ = self.st(self.attn_bwd(qkv_t, gC, s, j))
        gC = self.st(gQ @ self.wqkv(s, j)[0])
        return self.ln_bwd(xin, gC, b + "layernorm_before.weight", gR)

    def merge_bwd(self, m, gR, s):
        d = f"encoder.layers.{s}.downsample."
        gC = self.st(self.st(self.x(gR)) @ self.w(d + "reduction.weight"))
        return scatter_perm(self.ln_bwd(m, gC, d + "norm.weight"))

    def embed_ln_bwd(self, e0, gR):
        return self.ln_bwd(e0, gR, "embeddings.norm.weight")

    def embed_bwd(self, gF):
        n = gF.shape[0]
        g = self.x(gF) @ self.f("embeddings.patch_embeddings.projection.weight").reshape(96, 48)      # [n, 3136, 48]
        return g.reshape(n, 56, 56, 3, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(n, 3, 224, 224)


# ---- the cases of the gate, in the order they run on one handle (long ones first) ----
CASES = ("full", "three", "pair_edge", "one")
BF16_CASES = ("three", "pair_edge", "one")
GRAD_CASES = {"three": 2, "one": 1}            # case -> n_grad


def case(name):
    """-> (src_a, src_b or None, crops [(source index, y0, x0)]); fp32 sources in [0, 1)"""
    g = torch.Generator().manual_seed(11)
    if name == "full":
        return torch.rand(3, 3, 240, 250, generator=g), None, [(2, 16, 26), (0, 7, 0), (1, 0, 13), (0, 3, 5)]
    if name == "three":                          # the sources and crops of tests/test_gpu_swin.py
        return torch.rand(2, 3, 256, 272, generator=g), None, [(0, 5, 17), (1, 32, 48), (0, 0, 0)]
    if name == "pair_edge":                      # index crossing a -> b, odd row stride, unaligned x0, a crop flush bottom-right
        return torch.rand(1, 3, 230, 241, generator=g), torch.rand(2, 3, 230, 241, generator=g), [(2, 6, 17), (0, 0, 0), (1, 3, 1)]
    assert name == "one"
    return torch.rand(1, 3, 224, 224, generator=g), None, [(0, 0, 0)]


def crops_of(name):
    """[n, 3, 224, 224] fp32: the crops the device cuts out"""
    a, b, crops = case(name)
    src = a if b is None else torch.cat([a, b])
    return torch.stack([src[i, :, y:y + 224, x:x + 224] for i, y, x in crops])
