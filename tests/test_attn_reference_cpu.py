"""CPU checks of the operator gate of the window attention (tests/attn_ref.py): the explicit forward / backward restatement equals
the oracle, its bf16 emulation reproduces the oracle's own, the comparator rejects eight one-line faults at 3x the bf16 budget in
every cell of the GPU test's matrix (tests/test_gpu_attn_ops.py), and no cell is so ill-conditioned that the budget hides them."""
import functools
import math

import pytest
import torch

from oracle import m2trans_oracle as O
from tests import attn_ref as A

CELLS = [(C, geo, reg) for C in A.CHANNELS for geo in A.GEOMETRIES for reg in A.REGIMES]
CELL_IDS = [f"C{C}-{B}x{h}x{w}-{reg}" for C, (B, h, w), reg in CELLS]
cells = pytest.mark.parametrize("C,geo,regime", CELLS, ids=CELL_IDS)


@functools.lru_cache(maxsize=4)      # the checks of a cell run back to back (test_cell below): each cell is evaluated once
def _cell(C, geo, regime, seed):
    """(inputs as the bf16 kernels see them, fp64 reference, bf16 budget)."""
    inp = A.make_inputs(C, *geo, regime, seed, "bf16")
    ref = A.reference(inp)
    return inp, ref, A.budget(inp, ref, C)


def _check_restatement_equals_oracle_fp64(C, geo, regime):
    """explicit() without rounding, in float64, against O.window_attention_core + autograd: <= 1e-12 of own norm, whole tensor and
    every pixel class."""
    for seed in A.SEEDS:
        inp, ref, _ = _cell(C, geo, regime, seed)
        err = A.errors(A.explicit(inp), ref)
        assert max(err.values()) <= 1e-12, {k: v for k, v in err.items() if v > 1e-12}


def _check_emulation_reproduces_oracle_emu(C, geo, regime):
    """With only K^ and P rounded, explicit() is the oracle's bf16 emulation (emu=_Emu(): straight-through gradient, which is what
    the explicit backward formulas with the fp32 P in delta / dS and the rounded P in dV state)."""
    for seed in A.SEEDS:
        inp, _, _ = _cell(C, geo, regime, seed)
        want = A.reference(inp, emu=O._Emu())
        err = A.errors(A.explicit(inp, A.POINTS_ORACLE_EMU), want)
        assert max(err.values()) <= 1e-12, {k: v for k, v in err.items() if v > 1e-12}


def _check_conditioning_cap(C, geo, regime):
    """The whole-tensor bf16 budget stays <= 1e-2 of own norm (an input regime whose emulation alone exceeds it would hide the
    1 % mutants), no budget is zero, and the grid regime is what it claims: exact in bf16, raw logits beyond +-90, top key < 0.9."""
    for seed in A.SEEDS:
        inp, _, bud = _cell(C, geo, regime, seed)
        for t in A.TENSORS:
            assert 0.0 < bud[(t, "all")] <= A.CONDITIONING_CAP, (t, seed, bud[(t, "all")])
        assert all(b > 0.0 for b in bud.values())
        if regime == "grid":
            raw = A.make_inputs(C, *geo, regime, seed, "fp32")
            assert all(torch.equal(raw[n], inp[n]) for n in ("q", "k", "v", "gout")), "grid inputs must be exact in bf16"
            kh = A.to_key_windows(inp["k"].double()) + A.rel_bias(inp["rel_h"].double(), inp["rel_w"].double())
            assert torch.equal(A.bf16_round(kh), kh), "k + rel must be exact in bf16"
            S = torch.bmm(A.to_windows(inp["q"].double()), kh.transpose(1, 2)) * float(C) ** -0.5
            assert float(S.max()) > 90.0 and float(S.min()) < -90.0
            assert float(torch.softmax(S, -1).max()) < 0.9
        if regime == "kzero":
            assert float(inp["k"].abs().max()) == 0.0


def test_pixel_classes_partition():
    """Every pixel is in exactly one class of each family, and the class sizes are the closed forms: 4-covered pixels
    4 (nh - 1)(nw - 1) (all away from the border), image-border pixels 2 (h + w) - 4."""
    for _, h, w in A.GEOMETRIES:
        cls = A.pixel_classes(h, w)
        nh, nw = h // 8, w // 8
        for fam in ("q", "kv"):
            assert torch.equal(sum(m.long() for m in cls[fam].values()), torch.ones(h, w, dtype=torch.long))
        assert int(cls["kv"]["img_border"].sum()) == 2 * (h + w) - 4
        assert int(cls["kv"].get("cover4", torch.zeros(1)).sum()) == 4 * (nh - 1) * (nw - 1)
        n2 = 2 * ((nh - 1) * (w - 2) + (nw - 1) * (h - 2)) - 8 * (nh - 1) * (nw - 1)
        assert int(cls["kv"].get("cover2", torch.zeros(1)).sum()) == n2
        assert ("win_interior" in cls["q"]) == (nh > 2 and nw > 2)


# ------------------------------------------------------------------------------------------------ the gate discriminates
MUTANTS = ("key99_masked", "p_times_1.01", "phantom_masked", "no_rel_on_phantom", "drel_without_phantom", "fourth_overlap_dropped",
           "rel_halves_swapped", "strides_swapped")


def _noop(mutant, geo):
    """The ONLY cells where a mutant is not applied: where it is mathematically the identity."""
    _, h, w = geo
    if mutant == "strides_swapped":          # a [h][w] plane addressed as [w][h]: the same plane when h == w
        return h == w
    if mutant == "fourth_overlap_dropped":   # the diagonal window's ring row exists only where four windows meet: nh >= 2 and nw >= 2
        return h == 8 or w == 8
    return False


EXEMPT = {(m, geo) for m in MUTANTS for geo in A.GEOMETRIES if _noop(m, geo)}


def test_exemptions_are_exactly_the_noops():
    assert EXEMPT == {("strides_swapped", (1, 8, 8)), ("strides_swapped", (1, 24, 24)),
                      ("fourth_overlap_dropped", (1, 8, 8)), ("fourth_overlap_dropped", (1, 8, 16)),
                      ("fourth_overlap_dropped", (1, 16, 8)), ("fourth_overlap_dropped", (3, 8, 24))}


def _mutant_eval(inp, mutant=None):
    """A test-local fp64 copy of the reference (the forward of O.window_attention_core on the window gathers, gradients by autograd:
    each mutant comes with its own exact gradient, no rounding anywhere) with one fault switched on."""
    dt = torch.float64
    q, k, v = (inp[n].to(dt).clone().requires_grad_(True) for n in ("q", "k", "v"))
    rel_h, rel_w = (inp[n].to(dt).clone().requires_grad_(True) for n in ("rel_h", "rel_w"))
    gout = inp["gout"].to(dt)
    B, C, h, w = q.shape
    half = C // 2
    qq, kk, vv = q, k, v
    if mutant == "strides_swapped":          # window (wy, wx) / pixel (y, x) decomposed with h and w exchanged
        qq, kk, vv, gout = (t.reshape(B, C, w, h) for t in (q, k, v, gout))
        h, w = w, h
    qw, kw, vw = A.to_windows(qq), A.to_key_windows(kk), A.to_key_windows(vv)
    N = qw.shape[0]
    real = A.to_key_windows(torch.ones(1, 1, h, w, dtype=dt))[..., 0].bool().repeat(B, 1)           # [N, 100]: key inside the image
    kr, kc = torch.arange(100) // 10, torch.arange(100) % 10
    if mutant == "rel_halves_swapped":       # first C/2 channels <- rel_w[kc], last <- rel_h[kr]
        bias = torch.cat((rel_w[kc], rel_h[kr]), dim=-1)
    else:
        bias = A.rel_bias(rel_h, rel_w)
    bias = bias.unsqueeze(0).expand(N, 100, C)
    if mutant == "no_rel_on_phantom":
        bias = bias * real.unsqueeze(-1)
    if mutant == "drel_without_phantom":     # forward unchanged; the rel-pos gradient skips the phantom positions
        bias = torch.where(real.unsqueeze(-1), bias, bias.detach())
    if mutant == "fourth_overlap_dropped":   # forward unchanged; the ring rows of the window's four corner keys (the diagonal neighbour's
        corner = ((kr == 0) | (kr == 9)) & ((kc == 0) | (kc == 9))       # contribution to a 4-covered pixel) never reach dk | dv
        kw = torch.where(corner.view(1, 100, 1), kw.detach(), kw)
        vw = torch.where(corner.view(1, 100, 1), vw.detach(), vw)
    S = torch.bmm(qw, (kw + bias).transpose(1, 2)) * float(C) ** -0.5
    if mutant == "key99_masked":
        S = S.masked_fill((torch.arange(100) == 99).view(1, 1, 100), -math.inf)
    if mutant == "phantom_masked":           # phantom keys must TAKE softmax mass (value 0), not be masked out
        S = S.masked_fill(~real.unsqueeze(1), -math.inf)
    P = torch.softmax(S, dim=-1)
    if mutant == "p_times_1.01":
        P = P * 1.01
    out = A.from_windows(torch.bmm(P, vw), B, h, w)
    out.backward(gout)
    res = {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad, "drel_h": rel_h.grad, "drel_w": rel_w.grad}
    if mutant == "strides_swapped":
        res["out"] = res["out"].reshape(q.shape)
    return res


def _check_gate_accepts_budget_and_unmutated_copy(C, geo, regime):
    """The gate accepts the budget emulation itself (ratio 1 by construction: the comparator is wired to the right tensors) and
    the test-local copy with no mutant switched on (it IS the reference: <= 1e-12)."""
    for seed in A.SEEDS:
        inp, ref, bud = _cell(C, geo, regime, seed)
        bad, table = A.gate_bf16(A.explicit(inp, A.kernel_points(C)), ref, bud)
        assert not bad, bad
        assert all(abs(q - 1.0) < 1e-9 for _, _, q in table.values())
        err = A.errors(_mutant_eval(inp), ref)
        assert max(err.values()) <= 1e-12, err


def _check_gate_rejects_mutants(C, geo, regime):
    """Every mutant, in every cell where it is not the identity, exceeds 3x the bf16 budget in at least one whole-tensor or
    pixel-class entry (the max-norm metric is not counted).  -s prints mutant x cell: worst error / budget and where."""
    missed = []
    for seed in A.SEEDS:
        inp, ref, bud = _cell(C, geo, regime, seed)
        for m in MUTANTS:
            if (m, geo) in EXEMPT:
                err = A.errors(_mutant_eval(inp, m), ref)
                assert max(err.values()) <= 1e-12, (m, "listed as a no-op but is not", err)
                print(f"  C{C} {geo} {regime} seed {seed}  {m:24s} no-op in this cell (exempt)")
                continue
            _, table = A.gate_bf16(_mutant_eval(inp, m), ref, bud)
            (t, c), (e, b, ratio) = max(table.items(), key=lambda kv: kv[1][2])
            print(f"  C{C} {geo} {regime} seed {seed}  {m:24s} worst {t}[{c}] error {e:.2e} / budget {b:.2e} = {ratio:8.1f}")
            if not ratio > A.MARGIN:
                missed.append((m, seed, t, c, e, b))
    assert not missed, missed


CHECKS = {"restatement_equals_oracle_fp64": _check_restatement_equals_oracle_fp64,
          "emulation_reproduces_oracle_emu": _check_emulation_reproduces_oracle_emu,
          "conditioning_cap": _check_conditioning_cap,
          "gate_accepts_budget_and_unmutated_copy": _check_gate_accepts_budget_and_unmutated_copy,
          "gate_rejects_mutants": _check_gate_rejects_mutants}


@pytest.mark.parametrize("check", list(CHECKS))      # (the upper decorator varies fastest: cell by cell, check by check)
@cells
def test_cell(C, geo, regime, check):
    CHECKS[check](C, geo, regime)


def test_comparator_sees_a_pixel_class_fault():
    """A 1.2 % fault confined to the 4-covered pixels of dk (192 of 4608) is diluted in the whole-tensor norm and plain in its class."""
    C, geo = 64, (2, 32, 72)
    inp, ref, bud = _cell(C, geo, "randn", A.SEEDS[0])
    got = {t: x.clone() for t, x in A.explicit(inp, A.kernel_points(C)).items()}
    m = A.pixel_classes(*geo[1:])["kv"]["cover4"]
    got["dk"][..., m] *= 1.012
    _, table = A.gate_bf16(got, ref, bud)
    assert table[("dk", "all")][2] < A.MARGIN < table[("dk", "cover4")][2], (table[("dk", "all")], table[("dk", "cover4")])
