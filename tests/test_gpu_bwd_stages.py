"""-m gpu: teacher-forced stage gate of the backward pass -- every stored gradient of the default schedule against fp64.

The model runs through the autograd surface (lr.requires_grad_(True), loss (sr * w).sum() with a seeded random w, or L1 with part of the
output under the clamp) with DEFAULT plan options: in bf16 mode that is the fused path (the resident attention backward with the
projection data gradient inside it, c16_dgrad_prep, fused_prep_bwd / fused_norm_red, conv3x3_c64_bwd_rows, the fused tail backward).
tests/gpu_util.hip_backward_trace then reads the gradient taps back and tests/bwd_stage_ref.py judges each one against the VJP of the
run's own upstream tap through the float64 oracle (teacher-forced along the run's forward trajectory in bf16 mode), whole tensor and per
pixel class:
  bf16   every entry <= 3 x its budget (the explicit chain with the kernels' bf16 rounding points; lr.grad, an fp32 tensor: the head data
         gradient's 576-term fp32 accumulation chain).  Floor where the budget is exactly zero -- gpre alone: g(sr) times a 0 / 1 mask -- is the
         float32 oracle's own error against float64 on that stage, which is zero too: the seed must be bit-exact, and is;
  fp32   every entry <= 1e-4 of own norm, or <= 3 x the float32 oracle's own error.
Run with -s for each cell's table (error, budget, ratio per (tap, class)).

The gate's first device run found no kernel fault and one point missing from the emulation: with lr.grad's budget taken from the float32
oracle (a blocked sum, 2.3e-7 of own norm at 1x32x32) the head data gradient stood at 3.5x (8.0e-7; 7.2e-7 .. 1.3e-6 in every cell and both
compute types).  head_conv_dgrad_kernel sums its 576 products in one fp32 FMA chain; restated in that order the budget is 4.7e-7 .. 1.2e-6.

MEASURED on MI355X, worst over the cells below per (tap, class): bf16 = error / budget with (error, budget) and the cell; fp32 = error with
(the float32 oracle's own error) and the cell.  Cells are named <scale> nb<blocks> <B>x<H>x<W> [l1].
  tap        class       | bf16: worst error / budget (error, budget), cell          | fp32: worst error (float32 oracle's), cell
  g_t1pre    all         |  1.00 (2.1e-03, 2.1e-03) x4 nb1 1x32x32              | 8.8e-07 (8.5e-07) x4 nb2 2x40x56
  g_t1pre    border      |  1.16 (2.5e-03, 2.2e-03) x4 nb1 1x96x128             | 8.9e-07 (8.9e-07) x4 nb2 2x40x56
  g_t1pre    interior    |  1.00 (2.1e-03, 2.1e-03) x4 nb1 1x32x32              | 8.8e-07 (8.5e-07) x4 nb2 2x40x56
  gT         all         |  1.00 (1.6e-03, 1.6e-03) x4 nb1 1x32x32              | 7.4e-07 (3.7e-07) x4 nb1 2x40x56 l1
  gT         border      |  1.03 (3.3e-03, 3.2e-03) x3 nb1 2x40x56              | 6.5e-07 (7.2e-07) x2 nb1 2x40x56
  gT         interior    |  1.00 (1.6e-03, 1.6e-03) x4 nb1 1x32x32              | 7.6e-07 (3.7e-07) x4 nb1 2x40x56 l1
  b0.gqkv1   all         |  1.01 (4.3e-03, 4.3e-03) x4 nb1 1x32x32              | 1.5e-06 (2.7e-06) x4 nb1 2x40x56
  b0.gqkv1   img_border  |  1.04 (4.6e-03, 4.5e-03) x4 nb1 2x40x56              | 1.3e-06 (2.5e-06) x4 nb1 3x64x96
  b0.gqkv1   cover1      |  1.02 (5.3e-03, 5.3e-03) x4 nb1 2x40x56              | 1.5e-06 (2.9e-06) x4 nb1 2x40x56
  b0.gqkv1   cover2      |  1.02 (4.4e-03, 4.3e-03) x4 nb1 1x32x32              | 1.5e-06 (2.6e-06) x4 nb1 2x40x56
  b0.gqkv1   cover4      |  1.05 (4.5e-03, 4.3e-03) x4 nb1 1x32x32              | 1.7e-06 (3.0e-06) x4 nb1 2x40x56
  b0.gqkv2   all         |  1.03 (7.1e-03, 6.9e-03) x4 nb1 1x32x32              | 2.3e-06 (4.2e-06) x4 nb1 2x40x56
  b0.gqkv2   img_border  |  1.03 (7.0e-03, 6.7e-03) x4 nb1 1x32x32              | 2.2e-06 (4.1e-06) x4 nb1 1x96x128
  b0.gqkv2   cover1      |  1.03 (6.7e-03, 6.5e-03) x4 nb1 1x32x32              | 2.2e-06 (4.0e-06) x4 nb1 2x40x56
  b0.gqkv2   cover2      |  1.02 (7.7e-03, 7.6e-03) x4 nb1 1x32x32              | 2.4e-06 (4.4e-06) x4 nb1 2x40x56
  b0.gqkv2   cover4      |  1.06 (1.2e-02, 1.1e-02) x4 nb1 1x32x32              | 2.7e-06 (4.9e-06) x4 nb1 2x40x56
  b0.gqkv3   all         |  1.01 (2.1e-03, 2.1e-03) x4 nb1 2x40x56 l1           | 1.1e-06 (1.9e-06) x4 nb1 1x32x32
  b0.gqkv3   img_border  |  1.02 (3.2e-03, 3.2e-03) x2 nb1 2x40x56              | 1.1e-06 (1.9e-06) x4 nb1 1x32x32
  b0.gqkv3   cover1      |  1.02 (3.6e-03, 3.5e-03) x3 nb1 2x40x56              | 1.1e-06 (1.9e-06) x4 nb1 1x32x32
  b0.gqkv4   all         |  1.02 (2.6e-03, 2.6e-03) x2 nb1 2x40x56              | 9.0e-07 (1.5e-06) x4 nb1 1x32x32
  b0.gqkv4   img_border  |  1.03 (2.6e-03, 2.5e-03) x2 nb1 2x40x56              | 9.1e-07 (1.5e-06) x4 nb1 1x32x32
  b0.gqkv4   cover1      |  1.02 (2.5e-03, 2.4e-03) x2 nb1 2x40x56              | 9.0e-07 (1.5e-06) x4 nb1 1x32x32
  gn[1]      all         |  1.00 (3.5e-03, 3.5e-03) x4 nb1 1x32x32              | 1.0e-06 (3.8e-06) x4 nb1 2x40x56 l1
  gn[1]      img_border  |  1.03 (3.7e-03, 3.6e-03) x4 nb1 2x40x56              | 1.0e-06 (1.7e-06) x4 nb1 2x40x56
  gn[1]      cover1      |  1.00 (3.5e-03, 3.5e-03) x4 nb1 1x32x32              | 1.1e-06 (4.1e-06) x4 nb1 2x40x56 l1
  gn[1]      cover2      |  1.01 (3.6e-03, 3.6e-03) x4 nb1 1x32x32              | 1.0e-06 (1.0e-06) x3 nb1 2x40x56
  gn[1]      cover4      |  1.01 (3.7e-03, 3.6e-03) x4 nb1 2x40x56              | 1.0e-06 (9.8e-07) x3 nb1 2x40x56
  gn[2]      all         |  1.01 (3.8e-03, 3.7e-03) x4 nb1 1x32x32              | 1.3e-06 (4.8e-06) x4 nb1 2x40x56 l1
  gn[2]      img_border  |  1.06 (3.8e-03, 3.6e-03) x4 nb1 1x32x32              | 1.2e-06 (3.5e-06) x4 nb1 2x40x56 l1
  gn[2]      cover1      |  1.00 (3.8e-03, 3.8e-03) x4 nb1 1x32x32              | 1.3e-06 (4.8e-06) x4 nb1 2x40x56 l1
  gn[2]      cover2      |  1.01 (3.8e-03, 3.8e-03) x4 nb1 1x32x32              | 1.3e-06 (5.1e-06) x4 nb1 2x40x56 l1
  gn[2]      cover4      |  1.02 (4.1e-03, 4.0e-03) x4 nb1 1x32x32              | 1.3e-06 (4.4e-06) x4 nb1 2x40x56 l1
  gn[3]      all         |  1.00 (3.2e-03, 3.2e-03) x4 nb1 2x40x56              | 1.0e-06 (3.7e-06) x4 nb1 2x40x56 l1
  gn[3]      img_border  |  1.01 (3.2e-03, 3.2e-03) x4 nb1 1x96x128             | 1.0e-06 (3.4e-06) x4 nb1 2x40x56 l1
  gn[3]      cover1      |  1.00 (3.2e-03, 3.2e-03) x4 nb1 1x32x32              | 9.9e-07 (3.6e-06) x4 nb1 2x40x56 l1
  gn[4]      all         |  1.00 (2.4e-03, 2.4e-03) x4 nb1 2x40x56              | 7.6e-07 (2.8e-06) x4 nb1 2x40x56 l1
  gn[4]      img_border  |  1.01 (2.4e-03, 2.4e-03) x3 nb1 2x40x56              | 7.4e-07 (2.5e-06) x4 nb1 2x40x56 l1
  gn[4]      cover1      |  1.00 (2.3e-03, 2.4e-03) x4 nb1 2x40x56              | 7.6e-07 (2.9e-06) x4 nb1 2x40x56 l1
  gres       all         |  1.00 (2.2e-03, 2.2e-03) x4 nb1 1x32x32              | 4.4e-08 (4.3e-08) x4 nb2 2x40x56
  gres       border      |  1.02 (2.2e-03, 2.1e-03) x4 nb1 1x32x32              | 4.0e-08 (3.9e-08) x4 nb2 2x40x56
  gres       interior    |  1.00 (2.2e-03, 2.2e-03) x4 nb1 1x32x32              | 4.4e-08 (4.3e-08) x4 nb2 2x40x56
  gres       chan_mean   |  1.07 (3.0e-03, 2.8e-03) x4 nb2 2x40x56              | 3.3e-07 (3.5e-07) x4 nb1 2x40x56
  gres       along_xhat  |  1.04 (1.6e-03, 1.5e-03) x4 nb1 1x96x128             | 1.6e-07 (2.3e-07) x4 nb2 2x40x56
  lr.grad    all         |  1.54 (7.2e-07, 4.7e-07) x2 nb1 2x40x56              | 1.3e-06 (9.0e-07) x4 nb1 2x40x56 l1
  lr.grad    folded      |  1.70 (8.2e-07, 4.8e-07) x4 nb2 2x40x56              | 1.3e-06 (9.1e-07) x4 nb1 2x40x56 l1
  lr.grad    unfolded    |  1.00 (7.7e-07, 7.7e-07) x4 nb1 1x32x32              | 1.2e-06 (8.8e-07) x4 nb1 2x40x56 l1
  lr.grad    border      |  1.34 (5.6e-07, 4.2e-07) x2 nb1 2x40x56              | 9.5e-07 (5.9e-07) x4 nb1 2x40x56 l1
  lr.grad    interior    |  1.55 (7.3e-07, 4.7e-07) x2 nb1 2x40x56              | 1.3e-06 (9.3e-07) x4 nb1 2x40x56 l1
  gpre       all         |  0.00 (0.0e+00, 0.0e+00) x4 nb1 1x32x32              | 0.0e+00 (0.0e+00) x4 nb1 1x32x32
  b0.gqkv3   cover2      |  1.01 (2.3e-03, 2.3e-03) x4 nb1 2x40x56 l1           | 9.3e-07 (9.2e-07) x3 nb1 2x40x56
  b0.gqkv3   cover4      |  1.05 (3.1e-03, 3.0e-03) x2 nb1 2x40x56              | 9.9e-07 (1.8e-06) x4 nb1 1x96x128
  b0.gqkv4   cover2      |  1.02 (3.3e-03, 3.2e-03) x4 nb1 2x40x56              | 7.4e-07 (1.4e-06) x4 nb1 1x96x128
  b0.gqkv4   cover4      |  1.06 (2.7e-03, 2.6e-03) x2 nb1 2x40x56              | 8.0e-07 (1.5e-06) x4 nb1 1x96x128
  gn[3]      cover2      |  1.00 (3.2e-03, 3.2e-03) x4 nb1 2x40x56              | 1.0e-06 (3.8e-06) x4 nb1 2x40x56 l1
  gn[3]      cover4      |  1.03 (3.3e-03, 3.2e-03) x3 nb1 2x40x56              | 1.1e-06 (3.5e-06) x4 nb1 2x40x56 l1
  gn[4]      cover2      |  1.00 (2.4e-03, 2.4e-03) x4 nb1 2x40x56              | 7.6e-07 (3.0e-06) x4 nb1 2x40x56 l1
  gn[4]      cover4      |  1.01 (2.4e-03, 2.4e-03) x4 nb1 2x40x56              | 8.4e-07 (2.6e-06) x4 nb1 2x40x56 l1
  b1.gqkv1   all         |  1.00 (4.4e-03, 4.4e-03) x4 nb2 2x40x56              | 1.1e-06 (1.1e-06) x4 nb2 2x40x56
  b1.gqkv1   img_border  |  0.99 (4.1e-03, 4.2e-03) x4 nb2 2x40x56              | 1.0e-06 (1.2e-06) x4 nb2 2x40x56
  b1.gqkv1   cover1      |  1.00 (4.3e-03, 4.3e-03) x4 nb2 2x40x56              | 1.0e-06 (1.0e-06) x4 nb2 2x40x56
  b1.gqkv1   cover2      |  1.00 (4.5e-03, 4.5e-03) x4 nb2 2x40x56              | 1.1e-06 (1.1e-06) x4 nb2 2x40x56
  b1.gqkv1   cover4      |  0.98 (4.7e-03, 4.8e-03) x4 nb2 2x40x56              | 1.1e-06 (1.2e-06) x4 nb2 2x40x56
  b1.gqkv2   all         |  1.00 (5.2e-03, 5.2e-03) x4 nb2 2x40x56              | 1.3e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv2   img_border  |  0.99 (4.9e-03, 5.0e-03) x4 nb2 2x40x56              | 1.3e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv2   cover1      |  1.01 (4.7e-03, 4.6e-03) x4 nb2 2x40x56              | 1.2e-06 (1.6e-06) x4 nb2 2x40x56
  b1.gqkv2   cover2      |  1.00 (5.7e-03, 5.6e-03) x4 nb2 2x40x56              | 1.4e-06 (1.8e-06) x4 nb2 2x40x56
  b1.gqkv2   cover4      |  1.00 (6.1e-03, 6.0e-03) x4 nb2 2x40x56              | 1.3e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv3   all         |  1.01 (3.6e-03, 3.6e-03) x4 nb2 2x40x56              | 1.2e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv3   img_border  |  1.02 (3.5e-03, 3.5e-03) x4 nb2 2x40x56              | 1.4e-06 (2.1e-06) x4 nb2 2x40x56
  b1.gqkv3   cover1      |  1.01 (3.4e-03, 3.4e-03) x4 nb2 2x40x56              | 1.2e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv3   cover2      |  1.00 (3.8e-03, 3.8e-03) x4 nb2 2x40x56              | 1.1e-06 (1.8e-06) x4 nb2 2x40x56
  b1.gqkv3   cover4      |  1.01 (3.6e-03, 3.6e-03) x4 nb2 2x40x56              | 8.8e-07 (1.5e-06) x4 nb2 2x40x56
  b1.gqkv4   all         |  0.99 (3.0e-03, 3.0e-03) x4 nb2 2x40x56              | 1.2e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv4   img_border  |  0.99 (3.0e-03, 3.0e-03) x4 nb2 2x40x56              | 1.2e-06 (2.1e-06) x4 nb2 2x40x56
  b1.gqkv4   cover1      |  0.99 (2.8e-03, 2.9e-03) x4 nb2 2x40x56              | 1.3e-06 (1.9e-06) x4 nb2 2x40x56
  b1.gqkv4   cover2      |  0.99 (3.3e-03, 3.3e-03) x4 nb2 2x40x56              | 1.1e-06 (1.7e-06) x4 nb2 2x40x56
  b1.gqkv4   cover4      |  0.96 (3.1e-03, 3.3e-03) x4 nb2 2x40x56              | 8.8e-07 (1.1e-06) x4 nb2 2x40x56
  gB         all         |  1.00 (2.5e-03, 2.5e-03) x4 nb2 2x40x56              | 3.5e-07 (1.9e-07) x4 nb2 2x40x56
  gB         border      |  1.00 (2.3e-03, 2.4e-03) x4 nb2 2x40x56              | 2.8e-07 (1.7e-07) x4 nb2 2x40x56
  gB         interior    |  1.00 (2.6e-03, 2.6e-03) x4 nb2 2x40x56              | 3.6e-07 (1.9e-07) x4 nb2 2x40x56
"""
import pytest
import torch

from oracle import m2trans_oracle as O
from tests import bwd_stage_ref as R
from tests.gpu_util import build_model, hip_backward_trace, hip_forward_trace

pytestmark = pytest.mark.gpu


def _set(plan, key, value):
    from m2trans_amd import _lib
    _lib.check(_lib.load().m2t_set_option(plan.handle, key.encode(), int(value)), "m2t_set_option " + key)


def _step(model, x, w, hr):
    """One forward + backward through autograd (tests/test_gpu_input_grad.py _step); returns (lr.grad, sr, g(sr))."""
    model.zero_grad(set_to_none=True)
    lr = x.detach().clone().requires_grad_(True)
    sr = model(lr)
    seen = {}
    sr.register_hook(lambda g: seen.__setitem__("g_sr", g.detach().clone()))
    loss = (sr * w).sum() if w is not None else torch.nn.L1Loss()(sr, hr)
    loss.backward()
    torch.cuda.synchronize()
    return lr.grad.detach().clone(), sr.detach(), seen["g_sr"]


def _gate(scale, nb, B, H0, W0, dtype, loss_kind="smooth"):
    model, p = build_model(scale, nb, dtype)
    x = O.closed_form_image(B, 3, H0, W0)
    xd = x.cuda()
    w = hr = None
    if loss_kind == "smooth":
        w = R.cotangent(B, H0 * scale, W0 * scale).float().cuda()
    else:       # part of the output under the clamp (tests/test_gpu_input_grad.py)
        hr = (O.closed_form_image(B, 3, H0 * scale, W0 * scale, phase=0.7) * 1.2 - 0.1).clamp(0, 1).cuda()
    plan = model._plan_for(xd)
    H, W = plan.query("padded_h"), plan.query("padded_w")
    extra = {}
    if dtype == "bf16":
        # the default tails keep gelu / gelu' of their last expansion in LDS or registers; the stored-form run gives the same forward
        # bits (tests/test_gpu_baseline_configs.py check_vs_oracle) and its workspace feeds the teacher-forced oracle
        names, stored = (("t2act", "t2der"), 1) if scale == 4 else (("t1act", "t1der"), 0)
        if plan.query("stores_t2" if scale == 4 else "stores_t1") == 0:
            default = plan.query("opt:fused_tail")
            _set(plan, "fused_tail", stored)
            _, sr_stored, _ = _step(model, xd, w, hr)
            tr = hip_forward_trace(plan, scale, nb, B, H, W)
            extra = {n: tr[n] for n in names}
            _set(plan, "fused_tail", default)
            assert plan.query("stores_t2" if scale == 4 else "stores_t1") == 0
    gx, sr, g_sr = _step(model, xd, w, hr)
    if extra:
        assert torch.equal(sr, sr_stored), "the stored-form tail is not bit-identical in the forward pass"
    if loss_kind == "l1":
        assert bool(((sr <= 0) | (sr >= 1)).any())           # the clamp is live in this case
    ftrace = dict(hip_forward_trace(plan, scale, nb, B, H, W), **extra)
    taps = hip_backward_trace(plan, scale, nb, B, H, W)
    taps["lr.grad"] = gx.cpu()
    del model
    force = ftrace if dtype == "bf16" else None
    g64 = R.build_graph(x, p, scale, nb, dtype, force=force)
    g32 = R.build_graph(x, p, scale, nb, dtype, force=force, ftype=torch.float32)
    gpre_ref = R.seed(g_sr.cpu().double(), ftrace["srpre"].double())
    err, refs = R.stage_errors(g64, taps, gpre_ref)
    o32 = R.oracle32_errors(g64, g32, taps, refs, gpre_ref)
    required = {"gT", "gn[1]", "gn[2]", "gn[3]", "gn[4]", "b0.gqkv1", "b0.gqkv2", "b0.gqkv3", "b0.gqkv4", "gres", "lr.grad", "gpre"}
    required |= ({"g_t1pre"} if scale == 4 else set()) | ({"gB", "b1.gqkv1", "b1.gqkv2", "b1.gqkv3", "b1.gqkv4"} if nb == 2 else set())
    assert required <= {k[0] for k in err}, required - {k[0] for k in err}
    if dtype == "bf16":
        bad, table = R.gate_bf16(err, R.budget(g64, taps["gpre"]), floor=o32)
    else:
        bad, table = R.gate_fp32(err, o32)
    print(f"\nx{scale} nb={nb} {B}x{H0}x{W0} {dtype} {loss_kind}: error, " + ("budget, error / budget" if dtype == "bf16" else
                                                                               "float32 oracle's error, ratio"))
    print(R.format_table(table))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("B,H0,W0", [(1, 32, 32), (2, 40, 56), (3, 64, 96), (1, 96, 128)])
def test_x4_one_block(B, H0, W0, dtype):
    """1x32x32: a single level-2 window, every ring key a phantom; 2x40x56: reflect-padded to 64x64, 2x2 level-2 windows, pad fold live;
    3x64x96: odd B, 2x3; 1x96x128: 3x4, the first shape with an interior level-2 window."""
    _gate(4, 1, B, H0, W0, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_x4_one_block_l1_with_the_clamp_live(dtype):
    _gate(4, 1, 2, 40, 56, dtype, loss_kind="l1")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_x4_two_blocks(dtype):
    """The non-last block, the gB tap and buffer set 1."""
    _gate(4, 2, 2, 40, 56, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("scale", [2, 3])
def test_x2_x3_one_block(scale, dtype):
    """The streaming tails' gpre -> gT."""
    _gate(scale, 1, 2, 40, 56, dtype)
