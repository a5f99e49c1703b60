"""fp64 restatement of the TransBlock forward and of the eight backward steps of include/m2t_rlutrans.h, without autograd, and the
emulation of the bf16 route's rounding points.  TEST INFRASTRUCTURE ONLY: nothing here is on the product path.

``value_and_grads(x, params, gy, mask=None, bf16=False)`` returns ``(y, gx, grads, mask)``:

    forward    X -> Hn1 = LN1(X) -> R = Hn1 Wr^T -> QKV = R Wqkv^T -> AO = chunked attention -> X1 = AO Wp^T + bp + X
               -> Hn2 = LN2(X1) -> H1 = relu(Hn2 W1^T + b1) -> Y = H1 W2^T + b2 + X1
    backward   1 fc2   gH1 = (gy W2) * mask          dW2 = gy^T H1       db2 = colsum(gy)
               2 fc1   gHn2 = gH1 W1                 dW1 = gH1^T Hn2     db1 = colsum(gH1)
               3 LN2   gX1 = gy + LNbwd(gHn2; X1)    dgamma2 = colsum(gHn2 xhat1)   dbeta2 = colsum(gHn2)
               4 proj  gAO = gX1 Wp                  dWp = gX1^T AO      dbp = colsum(gX1)
               5 attention per (batch, chunk, head), scale 8^-1/2: delta = rowsum(gAO AO), gV = P^T gAO,
                       gS = P (gAO V^T - delta), gQ = scale gS K, gK = scale gS^T Q
               6 qkv   gR = gQKV Wqkv                dWqkv = gQKV^T R
               7 reduce gHn1 = gR Wr                 dWr = gR^T Hn1
               8 LN1   gx = gX1 + LNbwd(gHn1; X)     dgamma1, dbeta1

``mask`` [B, N, 16] (bool) forces the ReLU pattern: H1 = mask * (Hn2 W1^T + b1) in the forward and step 1 uses it.  With None the
mask is the forward's own, ``pre > 0``; forcing that same mask changes no bit.

``bf16=True`` applies a value -> bf16 -> value round trip wherever the bf16 route STORES a bf16 tensor (accumulation, softmax, the
LayerNorm statistics and every sum over tokens are fp32 on the device and are not rounding points):
    forward    the packed weight matrices, X, Hn1, R, QKV, AO, X1, Hn2, H1, Y        (biases and LayerNorm affine stay fp32)
    backward   gy as a GEMM operand (the residual use of gy stays fp32), gH1, gHn2, gX1 as a GEMM operand (the residual-stream
               copy of gX1 stays fp32), gAO, gQKV, gR, gHn1.  gx and all parameter gradients are fp32 outputs.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

Tensor = torch.Tensor
NAMES = ("atten.reduce.weight", "atten.qkv.weight", "atten.proj.weight", "atten.proj.bias", "norm1.weight", "norm1.bias",
         "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "norm2.weight", "norm2.bias")
SHAPES = ((2, 16), (2, 17), (2, 33), (2, 100), (3, 300))       # (3, 300): M = 900 rows leave 8 weight-gradient slabs (one per 128 rows)
# beyond the issue's five: the smallest N at which the attention backward takes its LDS-staged form (N // 16 >= 32) AND needs a second
# 64-token stage: chunks of 65 = stages of 64 + 1 = tiles of 32 + 32 + 1 rows, and a last chunk of 10
STAGED = (1, 1050)
EPS = 1e-5
SCALE = 8 ** -0.5


def rel(a: Tensor, b: Tensor) -> float:
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def inputs(B: int, N: int):
    """x and gy of the issue: torch.randn with a generator seeded by N."""
    g = torch.Generator().manual_seed(N)
    return torch.randn(B, N, 64, generator=g), torch.randn(B, N, 64, generator=g)


def _rt(t: Tensor, on: bool) -> Tensor:
    return t.to(torch.bfloat16).to(torch.float64) if on else t


def _ln_stats(x: Tensor):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS)
    return d * rstd, rstd


def _ln_bwd(g: Tensor, xhat: Tensor, rstd: Tensor, gamma: Tensor) -> Tensor:
    gg = g * gamma
    return rstd * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))


def _chunks(N: int):
    L = N // 16
    return [(j, min(N, j + L)) for j in range(0, N, L)]


def _heads(t: Tensor) -> Tensor:                     # [B, n, 64] -> [B, 8, n, 8]
    B, n, _ = t.shape
    return t.reshape(B, n, 8, 8).permute(0, 2, 1, 3)


def _tokens(t: Tensor) -> Tensor:                    # [B, 8, n, 8] -> [B, n, 64]
    B, _, n, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, 64)


def value_and_grads(x: Tensor, params: Dict[str, Tensor], gy: Tensor, mask: Optional[Tensor] = None, bf16: bool = False):
    p = {k: v.double() for k, v in params.items()}
    Wr, Wqkv, Wp, W1, W2 = (_rt(p[k], bf16) for k in ("atten.reduce.weight", "atten.qkv.weight", "atten.proj.weight", "mlp.fc1.weight",
                                                      "mlp.fc2.weight"))
    bp, b1, b2 = p["atten.proj.bias"], p["mlp.fc1.bias"], p["mlp.fc2.bias"]
    g1, be1, g2, be2 = p["norm1.weight"], p["norm1.bias"], p["norm2.weight"], p["norm2.bias"]
    r = lambda t: _rt(t, bf16)
    B, N, _ = x.shape
    # ---- forward
    X = r(x.double())
    xh, rs = _ln_stats(X)
    Hn1 = r(xh * g1 + be1)
    R = r(Hn1 @ Wr.T)
    QKV = r(R @ Wqkv.T)
    q, k, v = _heads(QKV[..., :64]), _heads(QKV[..., 64:128]), _heads(QKV[..., 128:])
    P = []
    AO = torch.empty(B, N, 64, dtype=torch.float64)
    for j0, j1 in _chunks(N):
        Pc = ((q[:, :, j0:j1] @ k[:, :, j0:j1].transpose(-2, -1)) * SCALE).softmax(-1)
        P.append(Pc)
        AO[:, j0:j1] = _tokens(Pc @ v[:, :, j0:j1])
    AO = r(AO)
    X1 = r(AO @ Wp.T + bp + X)
    x1h, rs1 = _ln_stats(X1)
    Hn2 = r(x1h * g2 + be2)
    pre = Hn2 @ W1.T + b1
    own = pre > 0
    if mask is None:
        mask = own
    H1 = r(pre * mask)
    Y = r(H1 @ W2.T + b2 + X1)
    # ---- backward
    gyd = gy.double()
    flat = lambda t: t.reshape(-1, t.shape[-1])
    G = {}
    gyT = r(gyd)
    gH1 = r((gyT @ W2) * mask)                                                   # 1
    G["mlp.fc2.weight"] = flat(gyT).T @ flat(H1)
    G["mlp.fc2.bias"] = flat(gyT).sum(0)
    gHn2 = r(gH1 @ W1)                                                           # 2
    G["mlp.fc1.weight"] = flat(gH1).T @ flat(Hn2)
    G["mlp.fc1.bias"] = flat(gH1).sum(0)
    gX1 = gyd + _ln_bwd(gHn2, x1h, rs1, g2)                                      # 3
    G["norm2.weight"] = flat(gHn2 * x1h).sum(0)
    G["norm2.bias"] = flat(gHn2).sum(0)
    gX1t = r(gX1)
    gAO = r(gX1t @ Wp)                                                           # 4
    G["atten.proj.weight"] = flat(gX1t).T @ flat(AO)
    G["atten.proj.bias"] = flat(gX1t).sum(0)
    gQKV = torch.empty(B, N, 192, dtype=torch.float64)                           # 5
    go, ao = _heads(gAO), _heads(AO)
    for (j0, j1), Pc in zip(_chunks(N), P):
        goc, qc, kc, vc = go[:, :, j0:j1], q[:, :, j0:j1], k[:, :, j0:j1], v[:, :, j0:j1]
        delta = (goc * ao[:, :, j0:j1]).sum(-1, keepdim=True)
        gS = Pc * (goc @ vc.transpose(-2, -1) - delta)
        gQKV[:, j0:j1, :64] = _tokens(SCALE * (gS @ kc))
        gQKV[:, j0:j1, 64:128] = _tokens(SCALE * (gS.transpose(-2, -1) @ qc))
        gQKV[:, j0:j1, 128:] = _tokens(Pc.transpose(-2, -1) @ goc)
    gQKV = r(gQKV)
    gR = r(gQKV @ Wqkv)                                                          # 6
    G["atten.qkv.weight"] = flat(gQKV).T @ flat(R)
    gHn1 = r(gR @ Wr)                                                            # 7
    G["atten.reduce.weight"] = flat(gR).T @ flat(Hn1)
    gx = gX1 + _ln_bwd(gHn1, xh, rs, g1)                                         # 8
    G["norm1.weight"] = flat(gHn1 * xh).sum(0)
    G["norm1.bias"] = flat(gHn1).sum(0)
    return Y, gx, {n: G[n] for n in NAMES}, mask


def oracle_grads(x: Tensor, params: Dict[str, Tensor], gy: Tensor):
    """fp64 autograd of oracle.rlutrans_oracle.trans_block: (y, gx, grads, relu mask)."""
    from oracle import rlutrans_oracle as RO
    import torch.nn.functional as F
    p = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    xd = x.double().clone().requires_grad_(True)
    y = RO.trans_block(xd, p)
    gs = torch.autograd.grad(y, [xd] + [p[n] for n in NAMES], gy.double())
    with torch.no_grad():
        x1 = xd + RO.eff_attention(F.layer_norm(xd, (64,), p["norm1.weight"], p["norm1.bias"], 1e-5), p)
        pre = F.linear(F.layer_norm(x1, (64,), p["norm2.weight"], p["norm2.bias"], 1e-5), p["mlp.fc1.weight"], p["mlp.fc1.bias"])
    return y.detach(), gs[0], dict(zip(NAMES, gs[1:])), pre > 0
