"""CPU only: the parameter-gradient half of the backward stage gate (tests/bwd_stage_ref.py param_refs / emulate / param_classes) checked
against itself before it judges a device run.  The consistency half -- chained references equal to autograd at 1e-12 for every
parameter -- is in tests/test_bwd_stage_reference_cpu.py next to the data taps.

  1. budget        the unfaulted emulation passes with every ratio <= 1; the one-kernel stages sit at the float32 floor, the stages with
                   a bf16 tensor between cotangent and parameter at a bf16-sized number;
  2. faults        one-line faults in the emulated parameter gradients fail the gate at the expected (parameter, class) and nowhere
                   but in that parameter (a parameter is a leaf: nothing lies downstream of it);
  3. the gap       which of these faults pass today's criterion (GRAD_REL / GRAD_OF_TOTAL of tests/test_gpu_baseline_configs.py): the
                   C = 256 branches' rel-pos and qkv-weight faults all do -- a table with rel_h and rel_w swapped, a window left out of
                   the sum, a weight gradient that lost its last slab.  That is why the gate exists.
"""
import functools

import pytest
import torch

from oracle import m2trans_oracle as O
from tests import attn_ref as A
from tests import bwd_stage_ref as R

GRAD_REL, GRAD_OF_TOTAL = 2e-2, 1e-5      # tests/test_gpu_baseline_configs.py check_vs_oracle

# 2x40x56 (padded to 64x64): level-2 M = 512 rows = 4 slabs of the C = 256 qkv weight gradient, 2x2 level-2 windows per image
CELL = (4, 1, 2, 40, 56, "bf16")
B0 = "body.0."


@functools.lru_cache(maxsize=None)
def _cell(scale, nb, B, H0, W0, dtype):
    p = O.closed_form_params(64, scale, nb)
    x = O.closed_form_image(B, 3, H0, W0)
    g = R.build_graph(x, p, scale, nb, dtype, leaf_params=True)
    g_sr = R.cotangent(B, H0 * scale, W0 * scale)
    return g, g_sr, R.seed(g_sr, g.cap["srpre"].detach())


@functools.lru_cache(maxsize=None)
def _budget(cell):
    g, _, gpre = _cell(*cell)
    return R.budget(g, gpre)


def _is_param(k):
    return k[0].startswith(("head.", "body.", "tail."))


# fault -> ((parameter, class) that must fail, the parameters that may fail)
def _expect():
    e = {}
    for i in range(4):
        w, rh, rw = (B0 + f"attn{i + 1}.{n}" for n in ("qkv_conv.weight", "rel_h", "rel_w"))
        e[f"wgrad_tail_rows:{i}"] = ((w, "k"), (w,))
        e[f"rel_drop_window:{i}"] = ((rw if i == 0 else rh, "inner"), (rh, rw))
        e[f"rel_swap:{i}"] = ((rw, "ring"), (rh, rw))
    e["bias_one_slab"] = (("tail.0.bias", "phase3"), ("tail.0.bias",))
    e["tail0_phase_order"] = (("tail.0.weight", "phase1"), ("tail.0.weight", "tail.0.bias"))
    e["head_wgrad_zero_pad"] = (("head.weight", "edge"), ("head.weight",))
    e["ff_wgrad_tap_transposed"] = ((B0 + "feed_forward.0.weight", "edge"), (B0 + "feed_forward.0.weight",))
    return e


EXPECT = _expect()
# one window is 1 of 128 (level 0) and 1 of 32 (level 1) at 2x40x56, inside the tables' budget (2e-2: sums over every window, with
# cancellation); at 1x32x32 it is 1 of 16, 1 of 4 and, at level 2, the only one.  (At level 0 the window's share of rel_h is 7e-2 of the
# table's norm, under 3 x 2.8e-2: rel_w, at 4.7e-1, is the entry that must fail.)
FAULT_CELLS = {f"rel_drop_window:{i}": (4, 1, 1, 32, 32, "bf16") for i in range(4)}


def test_every_parameter_fault_has_an_expectation():
    assert set(EXPECT) == set(R.PARAM_FAULTS)


def test_wgrad_slabs_restates_the_launcher():
    """launch_wgrad_tn (csrc/k_gemm.hip): 512 / (tiles of 64 x 64) slabs at most, one per 128 rows at most, whole slabs per XCD above 8."""
    assert R.wgrad_slabs(512, 768, 256) == (4, 128)          # C = 256 qkv at 2x16x16
    assert R.wgrad_slabs(1152, 768, 256) == (5, 256)         # 3x64x96: 9 row blocks in 5 slabs, the last one partial
    assert R.wgrad_slabs(64, 768, 256) == (1, 128)           # 1x32x32: less than one row block
    assert R.wgrad_slabs(8192, 48, 16) == (64, 128)          # C = 16
    assert R.wgrad_slabs(1280, 48, 16) == (5, 256)           # above 8 slabs: a multiple of 8, then re-derived from the rows per slab


def test_unfaulted_emulation_passes_and_the_budget_has_the_expected_size():
    g, _, gpre = _cell(*CELL)
    bud = _budget(CELL)
    err, _ = R.stage_errors(g, R.emulate(g, gpre, points=True), gpre_ref=gpre)
    bad, table = R.gate_bf16(err, bud)
    assert not bad, bad
    assert all(q <= 1.0 for _, _, q in table.values()), R.format_table(table)
    names = set(O.trainable_names(g.p))
    assert names <= {k[0] for k in bud}, names - {k[0] for k in bud}
    # one kernel between the cotangent and the parameter, bf16 operands that both sides share, float32 accumulation: the float32 floor
    for n in [B0 + f"attn{i}.qkv_conv.weight" for i in range(1, 5)] + [B0 + "feed_forward.0.weight", B0 + "feed_forward.0.bias",
                                                                        "tail.0.weight", "tail.0.bias", "head.bias"]:
        assert bud[(n, "all")] < 5e-6, (n, bud[(n, "all")])
    # a bf16 tensor on the way: geff (last conv), geff and gt2 (tail.3), the attention's points (rel tables), hcols (head weight)
    for n in ["tail.6.weight", "tail.3.weight", "tail.3.bias", "head.weight"] + [B0 + f"attn{i}.rel_{a}" for i in range(1, 5) for a in "hw"]:
        assert 1e-4 < bud[(n, "all")] < 1e-1, (n, bud[(n, "all")])      # (the tables are sums over all windows with cancellation: 2e-2)


def test_budget_from_the_runs_own_taps_is_the_plain_budget_when_the_emulation_plays_the_run():
    """R.budget(g, gpre, taps) restates the rel-pos tables' stage from the run's own gy; with the emulated taps that is the same
    arithmetic on the same values: every entry is bit-equal to the plain budget."""
    cell = (4, 1, 1, 32, 32, "bf16")
    g, _, gpre = _cell(*cell)
    assert R.budget(g, gpre, R.emulate(g, gpre, points=True)) == _budget(cell)


@pytest.mark.parametrize("fault", R.PARAM_FAULTS)
def test_gate_rejects_parameter_fault_at_the_expected_entry_and_class(fault):
    cell = FAULT_CELLS.get(fault, CELL)
    g, _, gpre = _cell(*cell)
    bud = _budget(cell)
    (name, cls), allowed = EXPECT[fault]
    err, _ = R.stage_errors(g, R.emulate(g, gpre, points=True, fault=fault), gpre_ref=gpre)
    bad, table = R.gate_bf16(err, bud)
    failing = {k for k, (e, b, _) in table.items() if not e <= A.MARGIN * b}
    assert (name, cls) in failing, (fault, R.format_table({k: table[k] for k in table if k[0] == name}))
    stray = {k for k in failing if k[0] not in allowed}
    assert not stray, (fault, stray)
    assert any(f"{name}[{cls}]" in line for line in bad)


@pytest.mark.parametrize("shape", [(1, 32, 32), (2, 40, 56)])
def test_which_parameter_faults_pass_todays_criteria(shape):
    """Today's bf16 gate accepts a parameter tensor within GRAD_REL of its own norm OR within GRAD_OF_TOTAL of the whole gradient.
    EVERY rel-pos fault passes it, on every branch and at both shapes: the tables are 1e-7 .. 5e-6 of the whole gradient, so the second
    clause takes a table with rel_h and rel_w swapped (off by 1 .. 3.6x its own norm), one short of a window (3e-1 of its norm on the
    C = 256 branches at 2x40x56), and at 1x32x32 -- one level-2 window -- one that is simply zero.  wgrad_tail_rows passes it on the
    C = 16 and C = 64 branches at 2x40x56 (128 of 8192 / 1024 rows: 4e-4 / 9e-3 of the tensor's norm, first clause).  On the C = 256
    branches of these one-block cells it does NOT: there the last slab is a quarter of the rows (4e-1 of the norm) and the qkv weight
    gradient is 1e-3 of the whole gradient, so the lost slab is 4e-4 of it; it takes the depth of the shipped model, where
    tests/test_gpu_baseline_configs.py records these tensors at 3e-8 of the whole, for the second clause to cover it.  The bias, phase,
    padding and tap-order faults are large against both clauses.  The stage gate rejects all of them."""
    g, g_sr, gpre = _cell(4, 1, *shape, "fp32")
    full = R.autograd_param_grads(g, g_sr)
    total = float(torch.cat([v.reshape(-1) for v in full.values()]).norm())
    good = {n: v.detach() for n, v in R.emulate(g, gpre, points=False).items() if n in full}
    for n, v in full.items():                     # the emulation's parameter gradients are autograd's on the unfaulted chain
        assert A.own_norm_err(good[n].reshape(-1), v.reshape(-1)) <= 1e-10, n
    passes = {}
    for fault in R.PARAM_FAULTS:
        hurt = R.emulate(g, gpre, points=False, fault=fault)
        rows = [(n, float((hurt[n].detach() - good[n]).norm()) / float(good[n].norm()), float((hurt[n].detach() - good[n]).norm()) / total)
                for n in full]
        worst = max(rows, key=lambda r: min(r[1] / GRAD_REL, r[2] / GRAD_OF_TOTAL))
        assert worst[1] > 1e-6, (fault, worst)    # the fault is real (float64, no rounding points: an unfaulted tensor moves by 0)
        passes[fault] = all(r[1] < GRAD_REL or r[2] < GRAD_OF_TOTAL for r in rows)
        print(f"{fault} at {shape}: {worst[0]} off by {worst[1]:.1e} of its norm, {worst[2]:.1e} of the whole gradient: "
              + ("PASSES" if passes[fault] else "fails") + " today's rule")
    small = shape == (1, 32, 32)
    want = {f"{f}:{i}": True for f in ("rel_drop_window", "rel_swap") for i in range(4)}
    want.update({f"wgrad_tail_rows:{i}": (not small and i < 2) for i in range(4)})
    want.update({f: False for f in ("bias_one_slab", "tail0_phase_order", "head_wgrad_zero_pad", "ff_wgrad_tap_transposed")})
    assert passes == want, {f: (passes[f], want[f]) for f in want if passes[f] != want[f]}
