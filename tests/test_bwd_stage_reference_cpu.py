"""CPU only: the backward stage gate of tests/bwd_stage_ref.py checked against itself before it judges a device run.

  1. consistency   the stage references chained from the oracle's own seed, and the explicit chain without the kernels' rounding points,
                   reproduce plain torch.autograd.grad of the oracle to 1e-12 for every tap, lr.grad and every trainable parameter
                   (param_refs on the chained tap references; the parameter half's faults: tests/test_wgrad_stage_reference_cpu.py);
  2. faults        one-line faults injected into the emulated taps (which play the device) fail the gate at the expected (tap, class),
                   and only downstream of the faulted stage; the unfaulted emulation passes with every ratio <= 1;
  3. the gap       the three ring faults pass today's criteria (GRAD_REL / GRAD_OF_TOTAL per parameter tensor, lr.grad rel-rms 2e-2).
"""
import functools

import pytest
import torch

from oracle import m2trans_oracle as O
from tests import attn_ref as A
from tests import bwd_stage_ref as R
from tests.gpu_util import rms_rel

GRAD_REL, GRAD_OF_TOTAL, LR_RMS = 2e-2, 1e-5, 2e-2      # tests/test_gpu_baseline_configs.py, test_bf16_input_grad_vs_bf16_rounding_oracle


@functools.lru_cache(maxsize=None)
def _cell(scale, nb, B, H0, W0, dtype, leaf_params=False):
    p = O.closed_form_params(64, scale, nb)
    x = O.closed_form_image(B, 3, H0, W0)
    g = R.build_graph(x, p, scale, nb, dtype, leaf_params=leaf_params)
    g_sr = R.cotangent(B, H0 * scale, W0 * scale)
    return g, g_sr, R.seed(g_sr, g.cap["srpre"].detach())


# ------------------------------------------------------------------ 1. consistency
@pytest.mark.parametrize("shape", [(1, 32, 32), (1, 40, 56)])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("scale", [4, 2, 3])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_chained_stage_references_reproduce_autograd(dtype, scale, nb, shape):
    g, g_sr, gpre = _cell(scale, nb, *shape, dtype, True)
    want = R.autograd_taps(g, g_sr)
    chained = R.stage_refs(g, {"gpre": gpre}, chain=True)
    assert set(chained) == set(want)
    # the parameter gradients: param_refs with the chained tap references as cotangents, and the explicit chain's own
    want_p = R.autograd_param_grads(g, g_sr)
    chained_p = R.param_refs(g, dict(chained, gpre=gpre))
    assert set(chained_p) == set(want_p) == set(O.trainable_names(g.p))
    want = dict(want, **want_p)
    for what, got in (("stage references, chained", dict(chained, **chained_p)),
                      ("explicit chain, no rounding points", R.emulate(g, gpre, points=False))):
        err = R.errors(g, got, want)
        assert len(err) >= 20 and set(want_p) <= {k[0] for k in err}
        bad = {k: e for k, e in err.items() if not e <= 1e-12}
        assert not bad, (what, bad)


# ------------------------------------------------------------------ 2. faults
FAULT_CELL = (4, 1, 1, 40, 56, "bf16")
# image-corner windows are 4 of the 64 level-0 windows at 40x56 (padded to 64x64) and 4 of 16 at 32x32: the C = 16 corner fault is
# shown where it is a quarter of the windows (at 64x64 it stays under the margin: 1.3x the budget on cover2 / cover4)
FAULT_CELLS = {"ring_corner:0": (4, 1, 1, 32, 32, "bf16")}
# fault -> ((tap, class) that must fail, prefixes of the entries that may fail: the faulted stage's own tap and what lies downstream of it
# BEFORE the next teacher-forced tap)
EXPECT = {
    "ring:0": (("gn[1]", "cover2"), ("gn[1]",)),
    "ring:1": (("gn[2]", "cover2"), ("gn[2]", "gn[1]", "b0.gqkv1")),
    "ring:2": (("gn[3]", "cover2"), ("gn[3]", "gn[2]", "gn[1]", "b0.gqkv1", "b0.gqkv2")),
    "ring_corner:0": (("gn[1]", "cover4"), ("gn[1]",)),
    "ring_corner:1": (("gn[2]", "cover2"), ("gn[2]", "gn[1]", "b0.gqkv1")),
    "ring_corner:2": (("gn[3]", "cover2"), ("gn[3]", "gn[2]", "gn[1]", "b0.gqkv1", "b0.gqkv2")),
    "no_half:3": (("gn[4]", "all"), ("gn[", "b0.gqkv1", "b0.gqkv2", "b0.gqkv3")),
    "haar_sign:1": (("gn[2]", "all"), ("gn[2]", "gn[1]", "b0.gqkv1")),
    "in_no_xhat_term": (("gres", "along_xhat"), ("gres",)),
    "res_once": (("gres", "all"), ("gres",)),
    "conv_border_row": (("gn[1]", "img_border"), ("gn[", "b0.gqkv")),
    "head_no_fold": (("lr.grad", "folded"), ("lr.grad",)),
    "tail_no_reflect": (("g_t1pre", "border"), ("g_t1pre",)),
}


@functools.lru_cache(maxsize=None)
def _budget(cell):
    g, _, gpre = _cell(*cell)
    return R.budget(g, gpre)


def test_every_fault_has_an_expectation():
    assert set(EXPECT) == set(R.FAULTS)


def test_unfaulted_emulation_passes_with_every_ratio_at_most_one():
    g, _, gpre = _cell(*FAULT_CELL)
    bud = _budget(FAULT_CELL)
    emu = R.emulate(g, gpre, points=True)
    err, _ = R.stage_errors(g, emu, gpre_ref=gpre)
    bad, table = R.gate_bf16(err, bud)
    assert not bad, bad
    assert all(q <= 1.0 for _, _, q in table.values()), R.format_table(table)
    # the budget is a bf16-sized number wherever a bf16 tensor lies between two taps, and exactly zero where none does
    for k in (("gT", "all"), ("gn[3]", "cover2"), ("gres", "all"), ("b0.gqkv1", "all"), ("g_t1pre", "border")):
        assert 1e-4 < bud[k] < 2e-2, (k, bud[k])
    # lr.grad is an fp32 tensor: its budget is the 576-term fp32 accumulation chain of the head's data gradient; the seed is exact
    assert 1e-7 < bud[("lr.grad", "all")] < 3e-6 and bud[("gpre", "all")] == 0.0


@pytest.mark.parametrize("fault", R.FAULTS)
def test_gate_rejects_fault_at_the_expected_tap_and_class(fault):
    cell = FAULT_CELLS.get(fault, FAULT_CELL)
    g, _, gpre = _cell(*cell)
    bud = _budget(cell)
    (tap, cls), allowed = EXPECT[fault]
    err, _ = R.stage_errors(g, R.emulate(g, gpre, points=True, fault=fault), gpre_ref=gpre)
    bad, table = R.gate_bf16(err, bud)
    failing = {k for k, (e, b, _) in table.items() if not e <= A.MARGIN * b}
    assert (tap, cls) in failing, (fault, R.format_table({k: table[k] for k in table if k[0] == tap}))
    stray = {k for k in failing if not k[0].startswith(allowed)}
    assert not stray, (fault, stray)
    assert any(f"{tap}[{cls}]" in line for line in bad)          # the failure text names the stage and the class


def test_ring_fault_on_a_single_window_is_no_fault():
    """32x32: one level-2 window, every ring key of the C = 256 branches is a phantom -- losing the ring rows changes nothing."""
    cell = (4, 1, 1, 32, 32, "bf16")
    g, _, gpre = _cell(*cell)
    a, b = R.emulate(g, gpre, points=True), R.emulate(g, gpre, points=True, fault="ring:2")
    assert torch.equal(a["gn"], b["gn"]) and torch.equal(a["lr.grad"], b["lr.grad"])


# ------------------------------------------------------------------ 3. the gap, pinned
def _param_grads(g, taps):
    """The parameter gradients that follow from a set of taps (one block): attention weights and rel-pos tables from gqkv / drel,
    the head from gres; every other tensor sits upstream of the body's data gradient and does not see a fault in it."""
    c, out = g.cap, {}
    for i in range(1, 5):
        out[f"body.0.attn{i}.qkv_conv.weight"] = torch.einsum("bnhw,bkhw->nk", taps[f"b0.gqkv{i}"], c[f"b0.d{i}"].detach())
        out[f"body.0.attn{i}.rel_h"], out[f"body.0.attn{i}.rel_w"] = taps[f"b0.drel{i}"]
    w = g.p["head.weight"].detach().clone().requires_grad_(True)
    bias = g.p["head.bias"].detach().clone().requires_grad_(True)
    y = O.conv3x3_reflect(O.pad_to_multiple(g.x.detach()), w, bias)
    out["head.weight"], out["head.bias"] = torch.autograd.grad(y, (w, bias), taps["gres"])
    return out


@pytest.mark.parametrize("branch", [0, 1, 2])
@pytest.mark.parametrize("shape", [(1, 32, 32), (1, 40, 56)])
def test_ring_faults_pass_todays_criteria(shape, branch):
    """Why the stage gate exists: with ALL ring rows of one branch's projection data gradient lost, every parameter-gradient tensor is
    within GRAD_REL of its norm or GRAD_OF_TOTAL of the whole gradient, and lr.grad within 2e-2 rel-rms -- today's bf16 gates."""
    g, g_sr, gpre = _cell(4, 1, *shape, "fp32", True)
    H0s, W0s = g.H0 * 4, g.W0 * 4
    loss = (torch.clamp(g.cap["srpre"][..., :H0s, :W0s], 0.0, 1.0) * g_sr).sum()
    names = O.trainable_names(g.p)
    full = dict(zip(names, torch.autograd.grad(loss, [g.p[n] for n in names], retain_graph=True)))
    total = float(torch.cat([v.reshape(-1) for v in full.values()]).norm())
    good = R.emulate(g, gpre, points=False)
    hurt = R.emulate(g, gpre, points=False, fault=f"ring:{branch}")
    pg, ph = _param_grads(g, good), _param_grads(g, hurt)
    for n in pg:                                  # the helper is right: it reproduces autograd on the unfaulted taps
        assert A.own_norm_err(pg[n].reshape(-1), full[n].reshape(-1)) <= 1e-10, n
    rows = [(n, float((ph[n] - pg[n]).detach().norm()) / float(pg[n].detach().norm()), float((ph[n] - pg[n]).detach().norm()) / total) for n in pg]
    lr_rms = rms_rel(hurt["lr.grad"], good["lr.grad"])
    print(f"ring:{branch} at {shape}: lr.grad rel-rms {lr_rms:.2e}; worst tensor " + ", ".join(
        f"{n} {a:.1e}/{t:.1e}" for n, a, t in sorted(rows, key=lambda r: -min(r[1] / GRAD_REL, r[2] / GRAD_OF_TOTAL))[:2]))
    if shape == (1, 40, 56):
        assert lr_rms > 1e-4                      # the fault is real at this shape (at 32x32 the level-2 branches have no ring)
    assert lr_rms <= LR_RMS
    bad = [r for r in rows if not (r[1] < GRAD_REL or r[2] < GRAD_OF_TOTAL)]
    assert not bad, bad
