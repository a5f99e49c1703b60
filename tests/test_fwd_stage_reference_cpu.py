"""CPU only: the forward stage gate of tests/fwd_stage_ref.py checked against itself before it judges a device run.

  1. consistency   the stage references chained from the input reproduce oracle.m2trans_oracle.forward in float64 to 1e-12 for every stored
                   tensor, srpre and sr, at every cell of tests/test_gpu_fwd_stages.py;
  2. self-gate     with the emulation playing the device every ratio error / budget is exactly 1 (its stages restated from its own
                   taps give the same bits), and the gate's table holds exactly the required (stage, class) entries of the cell;
  3. faults        every entry of FAULTS fails the gate at the expected (stage, class) and nowhere outside the faulted stage's reach.
                   The H / W swap of the pixel shuffle is flagged at 1x72x24 (padded to 96x32) and changes no bit at 1x32x32: the square cells of
                   check_vs_oracle could not have seen it.
"""
import functools

import pytest
import torch

from oracle import m2trans_oracle as O
from tests import attn_ref as A
from tests import fwd_stage_ref as R

# (scale, blocks, B, H0, W0): the cells of tests/test_gpu_fwd_stages.py
CELLS = [(4, 1, 1, 32, 32), (4, 1, 2, 40, 56), (4, 1, 3, 64, 96), (4, 1, 1, 96, 128), (4, 1, 1, 96, 96), (4, 1, 2, 72, 24),
         (4, 2, 2, 40, 56), (2, 1, 2, 40, 56), (3, 1, 2, 40, 56), (2, 1, 2, 72, 24), (3, 1, 2, 72, 24)]
ALL_QKV = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def _cell(scale, nb, B, H0, W0, dtype="bf16", stored_qkv=None, gain=1.0):
    return R.geometry(O.closed_form_image(B, 3, H0, W0), O.closed_form_params(64, scale, nb, gain=gain), scale, nb, dtype,
                      stored_qkv=stored_qkv)


@functools.lru_cache(maxsize=None)
def _self_gate(cell, dtype="bf16", stored_qkv=None):
    g = _cell(*cell, dtype, stored_qkv)
    taps = R.emulate(g)
    return (g, taps) + R.gate(g, taps)


# ------------------------------------------------------------------ 1. consistency
@pytest.mark.parametrize("cell", CELLS, ids=str)
def test_chained_reference_reproduces_the_oracle_forward(cell):
    scale, nb = cell[:2]
    g = _cell(*cell, "fp32")                                     # (every q | k | v is an output)
    cap = {}
    sr = O.forward(g.x.double(), {k: v.double() for k, v in g.p.items()}, scale, nb, cap=cap)
    want = {n: cap[n] for n in cap if not n.endswith(("xn", "t1pre"))}
    want["sr"] = sr
    got = R.reference(g, chain=True)
    assert set(want) <= set(got) and set(got) - set(want) == {f"b{b}.{s}" for b in range(nb) for s in ("mean", "rstd")}
    for n, w in want.items():
        assert got[n].dtype == torch.float64 and got[n].shape == w.shape, n
        assert A.own_norm_err(got[n], w) <= 1e-12, (n, A.own_norm_err(got[n], w))
    # the clamp is live at every cell with the closed-form weights
    crop = cap["srpre"][..., :g.H0 * scale, :g.W0 * scale]
    assert bool(((crop < 0) | (crop > 1)).any())


# ------------------------------------------------------------------ 2. the emulation through its own gate
@pytest.mark.parametrize("cell", CELLS, ids=str)
def test_emulation_playing_the_device_has_every_ratio_exactly_one(cell):
    g, taps, bad, table, err = _self_gate(cell)
    assert not bad, bad
    assert set(table) == R.required_entries(g), set(table) ^ R.required_entries(g)
    off = {k: v for k, v in table.items() if not (v[2] == 1.0 or (k[0] == "sr" and v[0] == 0.0 and v[1] == 0.0))}
    assert not off, R.format_table(off)
    # a bf16-sized budget wherever a bf16 tensor is stored, a float32-sized one for the statistics and an exact sr
    for k in (("X0", "all"), ("b0.d3", "img_border"), ("b0.xc[2]", "win_corner"), ("X1", "border"), ("t1act", "all")):
        assert 1e-4 < table[k][1] < 2e-2, (k, table[k])
    assert 0 < table[("b0.rstd", "all")][1] < 1e-6 and table[("sr", "all")][1] == 0.0


def test_self_gate_with_every_qkv_stored_and_in_fp32():
    """q | k | v of branches 1 and 2 as stages of their own (fused_c16_fwd = fused_attn_fwd = 1), and the fp32 gate on the float32 oracle."""
    cell = (4, 1, 2, 40, 56)
    g, _, bad, table, _ = _self_gate(cell, "bf16", ALL_QKV)
    assert not bad and set(table) == R.required_entries(g)
    assert {("b0.qkv1", "cover4"), ("b0.qkv2", "pad")} <= set(table)
    assert all(v[2] == 1.0 for k, v in table.items() if k[0] != "sr")
    g, _, bad, table, _ = _self_gate(cell, "fp32")
    assert not bad and set(table) == R.required_entries(g)
    # the float32 oracle IS the emulation without points, but for the statistics' restated accumulation order (and what normalises by them)
    exact = [v for k, v in table.items() if k[0] in ("X0", "X1", "t1act", "t1der", "t2act", "t2der", "srpre", "sr") or ".qkv" in k[0]]
    assert len(exact) >= 40 and all(v[0] == v[1] for v in exact)
    assert all(v[0] <= R.FP32_TOL for v in table.values())


# ------------------------------------------------------------------ 3. faults
FAULT_CELL = (4, 1, 1, 40, 56)          # padded to 64 x 64; 2 x 2 level-2 windows, every one an image corner
# the pixel shuffle works on the PADDED plane: 72 x 24 is padded to 96 x 32.  The phantom keys' rel-pos term is below the bf16 noise of a
# slice at the closed-form weights' logit scale (fwd_stage_ref, FAULTS): shown at twice the weights
FAULT_CELLS = {"shuffle_hw_swap": (4, 1, 1, 72, 24), "phantom_no_rel:0": FAULT_CELL + ("bf16", None, 2.0),
               "phantom_no_rel:1": FAULT_CELL + ("bf16", None, 2.0)}
# fault -> ((stage, class) that must fail, prefixes of the entries that may fail: the faulted stage, and the stages that restate the
# faulted value from their own upstream taps -- the residual xin of a slice, the normalised planes)
EXPECT = {
    "trunc:X1": (("X1", "chan_mean"), ("X1",)),
    "phantom_no_rel:0": (("b0.xc[1]", "chan_mean"), ("b0.xc[1]",)),
    "phantom_no_rel:1": (("b0.xc[2]", "chan_mean"), ("b0.xc[2]",)),
    "haar_sign:1": (("b0.d2", "all"), ("b0.d2",)),
    "no_half:2": (("b0.d3", "all"), ("b0.d3", "b0.xc[3]")),
    "pad_replicate": (("X0", "pad"), ("X0",)),
    "stats_unpadded": (("b0.mean", "all"), ("b0.mean", "b0.rstd", "b0.d", "b0.xc")),
    "last_conv_zero_pad": (("srpre", "border"), ("srpre",)),
    "shuffle_hw_swap": (("t1act", "all"), ("t1act", "t1der")),
    "crop_corner": (("sr", "all"), ("sr",)),
}


def test_every_fault_has_an_expectation():
    assert set(EXPECT) == set(R.FAULTS)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_gate_rejects_fault_at_the_expected_stage_and_class(fault):
    g = _cell(*FAULT_CELLS.get(fault, FAULT_CELL))
    (stage, cls), allowed = EXPECT[fault]
    bad, table, _ = R.gate(g, R.emulate(g, fault=fault))
    failing = {k for k, (e, b, _) in table.items() if not e <= A.MARGIN * b}
    assert (stage, cls) in failing, (fault, R.format_table({k: table[k] for k in table if k[0] == stage}))
    stray = {k for k in failing if not k[0].startswith(allowed)}
    assert not stray, (fault, stray)
    assert any(f"{stage}[{cls}]" in line for line in bad)        # the failure text names the stage and the class


def test_truncation_hides_from_the_whole_tensor_error():
    """Why chan_mean is a class: truncation doubles a pixel's rounding error (2x the budget, inside the margin) but biases every plane."""
    g = _cell(*FAULT_CELL)
    _, table, _ = R.gate(g, R.emulate(g, fault="trunc:X1"))
    assert table[("X1", "all")][2] <= A.MARGIN < table[("X1", "chan_mean")][2]


def test_pixel_shuffle_hw_swap_is_invisible_at_the_square_cell():
    g = _cell(4, 1, 1, 32, 32)
    good, hurt = R.emulate(g), R.emulate(g, fault="shuffle_hw_swap")
    assert all(torch.equal(good[n], hurt[n]) for n in good)
    bad, _, _ = R.gate(g, hurt)
    assert not bad
