"""Stage-level gate of the MedCLIP text tower (csrc/m2t_text.hip): fp64 restatement per stage, bf16 emulation, metric, cases.

Plain helper module (CPU only, no pytest hooks), shared by tests/test_text_ref_cpu.py and tests/test_gpu_text_stages.py.

STAGES, in the order m2t_text_encode_ex launches them (rows = n * len token rows, row-major [n][len][...]):
  embed      X   = LayerNorm(word[id] + type[0] + pos[t]), t = row % len                       text_embed_kernel
  per layer l:
    qkv      QKV = X Wqkv^T + bqkv                      [rows][q | k | v = 3 x 768]             GEMM, BIAS epilogue
    attn     AO  = softmax(q k^T / 8 over the attended keys) v, 12 heads x 64                  text_attn_kernel
    attn_out XM  = LayerNorm(Y'),  Y' = AO Wo^T + bo + X                                       GEMM BIAS_RESID, LayerNorm
    fc1      MH  = gelu_erf(XM W1^T + b1)               [rows][3072]                            GEMM BIAS_GELU
    fc2      Y   = MH W2^T + b2 + XM                                                           GEMM BIAS_RESID
    ln_out   X   = LayerNorm(Y)                         = hidden_states[l + 1]                  LayerNorm
  pool       pooled[seq] = sum over hidden states 1, 2, 12 of the UNMASKED token mean          text_pool_kernel (x 3)
  head       emb = normalise(P (pooled / 3))                                                   text_head_kernel

MASK RULE (stated once, ``attention_weights``): a key is attended iff mask != 0; a sequence with NO attended key gets uniform
weights 1 / len over its len keys (transformers' additive finfo.min mask absorbs every score there; oracle/text_oracle.py
does the same, and tests/test_text_ref_cpu.py pins this module to it on such a sequence).

BF16 EMULATION (``emu=True``).  The rounding points are read off the code, not off a run: X, XM, Y (both uses), QKV, AO, MH
and the packed GEMM weights (m2t_text_load_weights -> launch_convert) are stored as bf16; biases, LayerNorm parameters and the
three embedding tables are read as fp32; every GEMM, LayerNorm, softmax and mean accumulates in fp32 and rounds ONCE, at its
store; the attention probabilities (LDS, fp32), `pooled` and the head are fp32 and are not rounding points.  The emulation is
the fp64 stage with a value -> bf16 -> value round trip at exactly those points (fp32 accumulation is not emulated: it is
1e-7, three orders below a bf16 store).  ``emu=False`` is the plain fp64 stage on the fp32 parameter values.

METRIC (``row_err``): the largest per-row relative L2 error over the rows of the stage output, so one bad token is not
averaged away.  ``BUGS`` are emulated kernel faults for the discrimination test of tests/test_text_ref_cpu.py.
"""
from __future__ import annotations

import math

import torch

from oracle import text_oracle as T

H, HEADS, DH, FF, LAYERS, VOCAB = T.HIDDEN, T.HEADS, 64, T.FF, T.LAYERS, T.VOCAB
EPS = T.LN_EPS
FILLED = 1200                 # word rows 0 .. FILLED - 1 carry closed_form_text_params(FILLED); row VOCAB - 1 carries last_word_row()
FP32_TOL = 2e-5               # per stage, fp32 device value against fp64 (tests/test_gpu_rlutrans_grad.py, tests/test_rlutrans.py)
MARGIN = 3.0                  # bf16: device error <= MARGIN x emulation error (tests/attn_ref.py)
BUGS = ("last_key", "keys64", "pos", "masked_mean", "zero_rule", "gemm_row")
BUG_STAGE = {"last_key": "attn", "keys64": "attn", "pos": "embed", "masked_mean": "pool", "zero_rule": "attn", "gemm_row": "qkv"}


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def last_word_row() -> torch.Tensor:
    c = torch.arange(H, dtype=torch.float64)
    return (0.05 * (torch.sin(c * 0.37 + 1.1) + 0.5 * torch.sin(c * 2.2360679 + 0.3))).to(torch.float32)


def make_params() -> dict:
    """fp32 parameters by HF name; the word table is FULL size: closed-form rows 0 .. FILLED - 1 and VOCAB - 1, zeros between."""
    p = T.closed_form_text_params(FILLED)
    word = torch.zeros(VOCAB, H, dtype=torch.float32)
    word[:FILLED] = p["embeddings.word_embeddings.weight"]
    word[VOCAB - 1] = last_word_row()
    p["embeddings.word_embeddings.weight"] = word
    return p


class F64View(dict):
    """The fp32 parameters read as fp64, tensor by tensor on access (the word table stays fp32: indexing it and adding an
    fp64 tensor promotes the gathered rows) -- what oracle.text_oracle needs to evaluate in fp64 without a second copy."""

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        return v if k == "embeddings.word_embeddings.weight" else v.to(torch.float64)


def _f(p, name):
    return p[name].to(torch.float64)


def _w(p, name, emu):
    w = p[name].to(torch.float64)
    return bf16(w) if emu else w


def _st(t, emu):
    return bf16(t) if emu else t


def layer_norm(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * g + b


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def embed(ids, p, emu=False, bugs=()):
    """ids [n, len] -> X [n, len, 768]"""
    n, ln = ids.shape
    t = torch.arange(n * ln).reshape(n, ln) if "pos" in bugs else torch.arange(ln).expand(n, ln)
    x = p["embeddings.word_embeddings.weight"][ids.long()].to(torch.float64) + _f(p, "embeddings.token_type_embeddings.weight")[0] \
        + _f(p, "embeddings.position_embeddings.weight")[t]
    return _st(layer_norm(x, _f(p, "embeddings.LayerNorm.weight"), _f(p, "embeddings.LayerNorm.bias")), emu)


def qkv(x, p, l, emu=False, bugs=()):
    b = f"encoder.layer.{l}.attention.self."
    w = torch.cat([_w(p, b + nm + ".weight", emu) for nm in ("query", "key", "value")])
    bias = torch.cat([_f(p, b + nm + ".bias") for nm in ("query", "key", "value")])
    y = _st(x.to(torch.float64) @ w.T + bias, emu)
    if "gemm_row" in bugs:
        y = y.clone()
        y[-1, -1] = 0.0                                   # the last row never written (a zeroed buffer underneath)
    return y


def attention_weights(scores, mask, bugs=()):
    """scores [n, heads, len, len], mask [n, len] -> softmax weights under THE mask rule of this tower."""
    n, ln = mask.shape
    att = mask != 0
    if "keys64" in bugs:
        att = att.clone()
        att[:, 64:] = False
    if "last_key" in bugs:
        att = att.clone()
        for s in range(n):
            idx = torch.nonzero(att[s]).flatten()
            if len(idx):
                att[s, idx[-1]] = False
    none = ~att.any(dim=1)                                  # sequences with no attended key
    s = scores.masked_fill(~att[:, None, None, :], -math.inf)
    s[none] = 0.0                                           # uniform: 1 / len on each of the len keys
    w = torch.softmax(s, dim=-1)
    if "zero_rule" in bugs:
        w[none] = 0.0
    return w


def attn(qkv_t, mask, emu=False, bugs=()):
    """QKV [n, len, 2304], mask [n, len] -> AO [n, len, 768]"""
    n, ln, _ = qkv_t.shape
    q, k, v = (qkv_t.to(torch.float64)[..., i * H:(i + 1) * H].reshape(n, ln, HEADS, DH).transpose(1, 2) for i in range(3))
    w = attention_weights(q @ k.transpose(-1, -2) * 0.125, mask, bugs)
    return _st((w @ v).transpose(1, 2).reshape(n, ln, H), emu)


def attn_out(ao, x, p, l, emu=False):
    b = f"encoder.layer.{l}.attention.output."
    y = _st(ao.to(torch.float64) @ _w(p, b + "dense.weight", emu).T + _f(p, b + "dense.bias") + x.to(torch.float64), emu)
    return _st(layer_norm(y, _f(p, b + "LayerNorm.weight"), _f(p, b + "LayerNorm.bias")), emu)


def fc1(xm, p, l, emu=False):
    b = f"encoder.layer.{l}.intermediate.dense."
    return _st(gelu_erf(xm.to(torch.float64) @ _w(p, b + "weight", emu).T + _f(p, b + "bias")), emu)


def fc2(mh, xm, p, l, emu=False):
    b = f"encoder.layer.{l}.output.dense."
    return _st(mh.to(torch.float64) @ _w(p, b + "weight", emu).T + _f(p, b + "bias") + xm.to(torch.float64), emu)


def ln_out(y, p, l, emu=False):
    b = f"encoder.layer.{l}.output.LayerNorm."
    return _st(layer_norm(y.to(torch.float64), _f(p, b + "weight"), _f(p, b + "bias")), emu)


def layer(x, mask, p, l, emu=False, bugs=()):
    """hidden_states[l] -> hidden_states[l + 1]"""
    xm = attn_out(attn(qkv(x, p, l, emu, bugs), mask, emu, bugs), x, p, l, emu)
    return ln_out(fc2(fc1(xm, p, l, emu), xm, p, l, emu), p, l, emu)


def hidden_states(ids, mask, p, emu=False, bugs=()):
    hs = [embed(ids, p, emu, bugs)]
    for l in range(LAYERS):
        hs.append(layer(hs[-1], mask, p, l, emu, bugs))
    return hs


def pool(h1, h2, h12, mask=None, bugs=()):
    """three hidden states [n, len, 768] -> pooled [n, 768]: the SUM of the three unmasked token means (fp32 on the device)"""
    out = 0.0
    for h in (h1, h2, h12):
        h = h.to(torch.float64)
        if "masked_mean" in bugs:
            m = (mask != 0).to(torch.float64)[..., None]
            out = out + (h * m).sum(1) / m.sum(1).clamp(min=1.0)
        else:
            out = out + h.mean(1)
    return out


def head(pooled, p):
    e = (pooled.to(torch.float64) / 3.0) @ _f(p, "projection_head.weight").T
    return e / e.norm(dim=-1, keepdim=True)


def encode(ids, mask, p, emu=False, bugs=()):
    hs = hidden_states(ids, mask, p, emu, bugs)
    return head(pool(hs[1], hs[2], hs[12], mask, bugs), p), hs


def row_err(got, want) -> float:
    """largest per-row relative L2 error; rows = everything but the last axis"""
    g, w = got.to(torch.float64).reshape(-1, got.shape[-1]), want.to(torch.float64).reshape(-1, want.shape[-1])
    return float(((g - w).norm(dim=1) / w.norm(dim=1).clamp(min=1e-300)).max())


# ---- the cases of the gate, in the order they run on one handle (long ones first) ----
CASES = ("max", "half+", "edge65", "edge64", "base", "allmasked", "short", "one")
BF16_CASES = ("half+", "edge64", "base", "allmasked", "short")
SHAPES = {"max": (1, 128), "half+": (2, 100), "edge65": (1, 65), "edge64": (2, 64), "base": (3, 19), "allmasked": (4, 7),
          "short": (1, 5), "one": (1, 1)}


def case(name):
    """-> (ids [n, len] int32, mask [n, len] int32)"""
    n, ln = SHAPES[name]
    g = torch.Generator().manual_seed(11 + CASES.index(name))
    ids = torch.randint(0, FILLED, (n, ln), generator=g, dtype=torch.int32)
    mask = torch.ones(n, ln, dtype=torch.int32)
    if name == "max":
        mask[0, -3:] = 0
        ids[0, 3], ids[0, 70], ids[0, 127] = 0, VOCAB - 1, VOCAB - 1
        ids[0, 64] = 0
    elif name == "half+":
        mask[1, 64:] = 0
    elif name == "edge64":
        mask[1, 0:2] = 0
        mask[1, 10:13] = 0
    elif name == "base":
        mask[2, 11:] = 0
    elif name == "allmasked":
        mask[2, :] = 0
    return ids, mask
