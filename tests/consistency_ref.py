"""fp64 restatement of the LR-consistency family (include/m2t_consistency.h), for the tests only.

Built on tests/imresize_ref.py -- MATLAB's general contributions form, NOT the kernel's tap table: the dense per-axis matrices
A_down(n) [n / s, n] and A_up(n) [n s, n] are that module's resize of the identity, and from them D x = A_H x A_W^T, the adjoint
D^T g = A_H^T g A_W, the loss, its gradient, one back-projection iteration and the statistics.  Every gradient / update comes with its
gate, per element q:

    2^-23 |ref(q)| + 2^-40 * coef * (|A_H|^T |g| |A_W|)(q)

the first part one fp32 rounding with a factor 2, the second the fp64 reordering of at most 16 x 16 products (and of the sums that
formed g) with a wide margin; an element of the update has the same form with |U|.  Values and statistics are sums of non-negative
terms: relative 1e-12.  Also the inputs the CPU and GPU tests share."""
import functools

import numpy as np

from tests import imresize_ref as ir

SCALES = (2, 3, 4)
LR_SHAPES = [(1, 1), (2, 3), (5, 7), (16, 32), (17, 33), (40, 56)]      # 16 x 32 is exactly one forward tile


@functools.lru_cache(maxsize=None)
def A_down(n: int, s: int) -> np.ndarray:
    """[n / s, n]: the down-sampler of one axis of length n (a multiple of s)."""
    return ir.resize_axis(np.eye(n, dtype=np.float64), 0, s, False)


@functools.lru_cache(maxsize=None)
def A_up(n: int, s: int) -> np.ndarray:
    """[n s, n]: the up-sampler of one axis of length n."""
    return ir.resize_axis(np.eye(n, dtype=np.float64), 0, s, True)


def down(x: np.ndarray, s: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return A_down(x.shape[-2], s) @ x @ A_down(x.shape[-1], s).T


def adjoint(g: np.ndarray, s: int) -> np.ndarray:
    g = np.asarray(g, dtype=np.float64)
    return A_down(g.shape[-2] * s, s).T @ g @ A_down(g.shape[-1] * s, s)


def adjoint_abs(g: np.ndarray, s: int) -> np.ndarray:
    g = np.abs(np.asarray(g, dtype=np.float64))
    return np.abs(A_down(g.shape[-2] * s, s)).T @ g @ np.abs(A_down(g.shape[-1] * s, s))


def up(r: np.ndarray, s: int) -> np.ndarray:
    r = np.asarray(r, dtype=np.float64)
    return A_up(r.shape[-2], s) @ r @ A_up(r.shape[-1], s).T


def up_abs(r: np.ndarray, s: int) -> np.ndarray:
    r = np.abs(np.asarray(r, dtype=np.float64))
    return np.abs(A_up(r.shape[-2], s)) @ r @ np.abs(A_up(r.shape[-1], s)).T


def stats_of(r: np.ndarray) -> np.ndarray:
    """{mean |r|, max |r|, mean r^2}"""
    return np.array([np.abs(r).mean(), np.abs(r).max(), (r * r).mean()], dtype=np.float64)


def loss_ref(x, y, s: int, R: float = 1.0, clamp: bool = True, eps: float = 0.0, scale: float = 1.0) -> dict:
    """x [..., H s, W s], y [..., H, W] (float32 values).  value = scale * sum rho(r); grad = dvalue / dx (fp64); gate per element of
    grad; r; stats; min_abs_r."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    cx = np.clip(x, 0.0, R) if clamp else x
    r = (down(cx, s) - y) / R
    if eps > 0.0:
        rho = np.sqrt(r * r + eps * eps)
        d = r / rho
    else:
        rho, d = np.abs(r), np.sign(r)
    mask = ((x >= 0.0) & (x <= R)).astype(np.float64) if clamp else np.ones_like(x)
    coef = scale / R
    grad = coef * mask * adjoint(d, s)
    gate = 2.0 ** -23 * np.abs(grad) + 2.0 ** -40 * abs(coef) * mask * adjoint_abs(d, s)
    return {"value": scale * rho.sum(), "grad": grad, "gate": gate, "r": r, "stats": stats_of(r), "min_abs_r": float(np.abs(r).min()),
            "mask": mask}


def back_project_ref(sr, lr, s: int, R: float = 1.0, beta: float = 1.0) -> dict:
    """One iteration from float32 values: r = (lr - D c(sr)) / R, its stats (the state BEFORE the update), new = clamp(fp32(sr + beta R
    U(r)), 0, R) as fp64 values before the rounding ("pre", and "new" = its clip), and the gate of an element of new."""
    sr = np.asarray(sr, dtype=np.float64)
    lr = np.asarray(lr, dtype=np.float64)
    r = (lr - down(np.clip(sr, 0.0, R), s)) / R
    pre = sr + beta * R * up(r, s)
    gate = 2.0 ** -23 * np.abs(pre) + 2.0 ** -40 * beta * R * up_abs(r, s)
    return {"r": r, "stats": stats_of(r), "pre": pre, "new": np.clip(pre, 0.0, R), "gate": gate}


def lr_psnr_ref(sr, lr, s: int, R: float = 1.0) -> float:
    r = (down(np.clip(np.asarray(sr, dtype=np.float64), 0.0, R), s) - np.asarray(lr, dtype=np.float64)) / R
    return float(-10.0 * np.log10((r * r).mean()))


# ----------------------------------------------------------------------------------------------------------- shared inputs
def loss_case(s: int, h: int, w: int, C: int, R: float = 1.0, B: int = 2):
    """(x [B,C,h s,w s], y [B,C,h,w]) float32: x spills over both ends of [0, R] and holds exact 0 and exact R."""
    rng = np.random.default_rng(1000 * s + 37 * h + w + C)
    y = (rng.uniform(0.0, 1.0, size=(B, C, h, w)) * R).astype(np.float32)
    x = (rng.uniform(-0.2, 1.2, size=(B, C, h * s, w * s)) * R).astype(np.float32)
    flat = x.reshape(B, C, -1)
    flat[:, :, 0] = 0.0                                                   # the ends of the range pass the mask
    flat[:, :, -1] = R
    if flat.shape[-1] > 8:
        flat[:, :, 5] = R
        flat[:, :, 7] = 0.0
    return x, y


def bp_case(s: int, h: int, w: int, C: int = 3, B: int = 2, clamp_active: bool = False):
    """(sr0 [B,C,h s,w s], lr [B,C,h,w]) float32, R = 1: the bicubic up-sampling of lr plus a perturbation.  clamp_active: lr reaches
    both ends of the range and the perturbation pushes sr0 beyond them."""
    rng = np.random.default_rng(7000 + 100 * s + 10 * h + w + C)
    lo, hi = (0.0, 1.0) if clamp_active else (0.25, 0.75)
    lr = rng.uniform(lo, hi, size=(B, C, h, w)).astype(np.float32)
    sr0 = up(lr, s) + 0.05 * rng.standard_normal(size=(B, C, h * s, w * s))
    return sr0.astype(np.float32), lr


BP_CASES = [(2, 5, 7, 3, False), (3, 17, 33, 1, False), (4, 16, 32, 3, False), (4, 12, 12, 3, True), (2, 1, 1, 1, False)]   # s, h, w, C, clamp
# the cases whose residual maximum falls at every one of four iterations at beta = 1 (tests/test_consistency_cpu.py checks it; the
# 1 x 1 case is consistent after ONE iteration and stays at the fp32 floor)
BP_MONOTONE = BP_CASES[:4]


def bp_run(sr0, lr, s: int, iters: int, beta: float, R: float = 1.0):
    """`iters` iterations in the restatement, each from the float32 rounding of the previous one: [stats of iteration k], final sr."""
    sr, rows = np.asarray(sr0, dtype=np.float32), []
    for _ in range(iters):
        o = back_project_ref(sr, lr, s, R, beta)
        rows.append(o["stats"])
        sr = np.clip(o["pre"].astype(np.float32), 0.0, R).astype(np.float32)
    rows.append(back_project_ref(sr, lr, s, R, beta)["stats"])
    return np.stack(rows), sr
