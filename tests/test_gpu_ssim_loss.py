"""-m gpu: the SSIM loss term (k_ssim_loss.hip; m2t_ssim_loss_tensor, m2t_ssim_loss, losses.ssim_loss, TrainStep(lambda_ssim=...))
against the fp64 restatement tests/ssim_loss_ref.py: the plan-free entry per element, the autograd Function, the plan entry on the
forward's own pre-clamp output, TrainStep against the sequence composed by hand and against the autograd route, the default step,
accumulation and the differentiable-SemanticLoss route.

The gate of a gradient element is |got - ref| <= 1e-6 |ref| + 1e-7 scale (scale = weight / divisor): the kernel differs from the
reference by the order of its fp64 sums and ONE fp32 rounding (6e-8); a wrong coefficient, a missing factor 2 or a wrong tap is off
by far more.  Where the destination held something before, the fp32 add contributes half an ulp of the sum: 6e-8 |prefill + ref|."""
import ctypes as C

import pytest
import torch

from oracle import m2trans_oracle as O
from tests import pixel_loss_ref as RP
from tests import ssim_loss_ref as R
from tests.gpu_util import assert_flat_equal
from tests.test_gpu_pixel_loss import _backward, _forward, _images, _model, _require_coverage, _srpre

pytestmark = pytest.mark.gpu

ARG, STATE = -2, -3
LAM = 0.1
HALF_ULP = 6e-8          # 2^-24 = 5.96e-8


def _lib_():
    from m2trans_amd import _lib
    return _lib, _lib.load()


def _scratch(lib, B, Cn, H, W, poison=False):
    n = lib.m2t_ssim_loss_scratch_bytes(B, Cn, H, W)
    assert n > 0
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    if poison:
        t.fill_(0xFF)
    return t


def _gate(got, ref, scale, prefill=None):
    """Elements beyond the gate (0 = pass), and the largest excess."""
    bound = 1e-6 * ref.abs() + 1e-7 * scale
    if prefill is not None:
        ref = prefill + ref
        bound = bound + HALF_ULP * ref.abs()
    excess = (got - ref).abs() - bound
    return int((excess > 0).sum()), float(excess.max())


# ------------------------------------------------------------------ 1. the plan-free entry against fp64
# (shape, phases of x and y, (rows, row stride) of the buffer that holds x or None = contiguous).  The phases are chosen so that the
# coverage condition below holds at every shape, the 11 x 11 one included.
CASES = [((1, 1, 11, 11), (0.3, 0.7), None),              # one map entry
         ((2, 3, 12, 43), (0.3, 1.9), None),              # a 2-row map, ragged
         ((1, 3, 75, 99), (0.3, 1.9), None),              # several tiles, tile seams in both axes
         ((2, 3, 40, 56), (0.3, 1.9), (48, 64))]          # strided x: row stride 64, image stride 3 * 48 * 64


def _tensor_inputs(shape, phases):
    B, Cn, H, W = shape
    x = (O.closed_form_image(B, Cn, H, W, phase=phases[0]) * 1.6 - 0.3).contiguous()
    y = O.closed_form_image(B, Cn, H, W, phase=phases[1]).contiguous()
    share = {"below 0": float((x < 0).double().mean()), "above 1": float((x > 1).double().mean()),
             "inside": float(((x >= 0) & (x <= 1)).double().mean())}
    assert min(share.values()) >= 0.05, f"{shape}: the inputs do not cover every class: {share}"
    return x, y


@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("shape,phases,layout", CASES, ids=["one-entry", "two-row-map", "tile-seams", "strided"])
def test_plan_free_entry_against_fp64(shape, phases, layout, clamp):
    _lib, lib = _lib_()
    B, Cn, H, W = shape
    x, y = _tensor_inputs(shape, phases)
    rows, rs = layout or (H, W)
    n_map = B * Cn * (H - 10) * (W - 10)
    scale = 0.37 / n_map
    want_loss, want = R.value_and_grad(x, y, 1.0, bool(clamp), scale)
    assert float(want.abs().max()) > 0
    nan = float("nan")
    xbuf = torch.full((B, Cn, rows, rs), nan)                       # what lies outside [H, W] must never be read ...
    xbuf[..., :H, :W] = x
    xbuf, yd = xbuf.cuda(), y.cuda()
    inside = torch.zeros((B, Cn, rows, rs), dtype=torch.bool)
    inside[..., :H, :W] = True
    g = torch.Generator().manual_seed(7)
    noise = (torch.randn((B, Cn, H, W), generator=g) * float(want.abs().max())).float()

    def run(prefill, loss_prefill, accumulate, scratch, with_grad=True):
        gbuf = torch.full((B, Cn, rows, rs), nan)                   # ... nor written
        gbuf[..., :H, :W] = prefill
        gbuf = gbuf.cuda()
        loss = torch.full((1,), loss_prefill, device="cuda")
        rc = lib.m2t_ssim_loss_tensor(_lib.ptr(xbuf), _lib.ptr(yd), B, Cn, H, W, Cn * rows * rs, rs, 1.0, clamp, scale,
                                      _lib.ptr(gbuf) if with_grad else None, _lib.ptr(loss), accumulate, _lib.ptr(scratch), _lib.stream_ptr())
        _lib.check(rc, "m2t_ssim_loss_tensor")
        torch.cuda.synchronize()
        return gbuf.cpu(), loss.cpu()

    tag = f"{shape} clamp {clamp}"
    g0, l0 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W))
    got = g0[..., :H, :W].double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l0).all()), tag
    nbad, worst = _gate(got, want, scale)
    print(f"{tag}: largest excess over the gate {worst:.3e} (max |ref| {float(want.abs().max()):.3e}, scale {scale:.3e})")
    assert nbad == 0, f"{tag}: {nbad} elements beyond the gate, worst by {worst:.3e}"
    if clamp:
        assert int(torch.count_nonzero(got[(x < 0) | (x > 1)])) == 0, f"{tag}: gradient where the clamp is active"
    # outside [H, W]: bit-unchanged
    assert torch.equal(g0.view(torch.int32)[~inside], torch.full((B, Cn, rows, rs), nan).view(torch.int32)[~inside]), tag
    # value
    print(f"{tag}: value {float(l0):.9e} against {float(want_loss):.9e}")
    assert abs(float(l0) - float(want_loss)) <= 1e-6 * abs(float(want_loss)), (tag, float(l0), float(want_loss))
    # two runs, and a run on NaN-poisoned scratch: bit-identical
    for poison in (False, True):
        g1, l1 = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W, poison))
        assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(l1, l0), (tag, poison)
    # value only: the same value
    _, lv = run(0.0, nan, 0, _scratch(lib, B, Cn, H, W), with_grad=False)
    assert torch.equal(lv, l0), tag
    # a prefilled destination is added to, in the gradient and (accumulate = 1) in the value
    g2, l2 = run(noise, 2.5, 1, _scratch(lib, B, Cn, H, W))
    nbad, worst = _gate(g2[..., :H, :W].double(), want, scale, prefill=noise.double())
    assert nbad == 0, f"{tag}: {nbad} elements of the prefilled destination beyond the gate, worst by {worst:.3e}"
    assert torch.equal(g2[..., :H, :W], noise + g0[..., :H, :W]), tag          # (the same fp32 add)
    assert torch.equal(l2, torch.tensor([2.5]) + l0), (tag, float(l2), float(l0))


# ------------------------------------------------------------------ 2. the autograd Function
def test_ssim_loss_function_gradient_and_errors():
    from m2trans_amd._lib import M2TError
    from m2trans_amd.losses import SSIMLoss, ssim_loss
    shape = (2, 3, 24, 40)
    x, y = _tensor_inputs(shape, (0.3, 1.9))
    leaf64 = x.double().requires_grad_(True)
    want = (1.0 - R.ssim_map(leaf64, y.double())).mean()
    want.backward()
    leaf = x.cuda().requires_grad_(True)
    got = ssim_loss(leaf, y.cuda())
    (got * 3.0).backward()                                          # (an upstream factor reaches the gradient)
    torch.cuda.synchronize()
    assert got.shape == () and abs(float(got) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
    scale = 1.0 / (2 * 3 * 14 * 30)
    nbad, worst = _gate(leaf.grad.double().cpu() / 3.0, leaf64.grad, scale)
    print(f"ssim_loss Function: largest excess over the gate {worst:.3e}")
    assert nbad == 0, (nbad, worst)
    assert float(SSIMLoss()(x.cuda(), y.cuda())) == float(got)
    with pytest.raises(M2TError):
        ssim_loss(x, y)                                             # host tensors: no fallback
    with pytest.raises(M2TError):
        ssim_loss(x[..., :10, :].cuda(), y[..., :10, :].cuda())      # a 10-row image
    with pytest.raises(M2TError):
        ssim_loss(x.cuda(), y.cuda().requires_grad_(True))


# ------------------------------------------------------------------ 3. the plan entry
def _n_map(hr):
    return hr.shape[0] * 3 * (hr.shape[-2] - 10) * (hr.shape[-1] - 10)


def _pixel(lib, plan, hr, out, weight=1.0, divisor=None, deferred=False):
    from m2trans_amd import _lib
    fn = lib.m2t_pixel_loss_deferred if deferred else lib.m2t_pixel_loss
    return fn(plan.handle, 0, 0.0, _lib.ptr(hr), weight, float(hr.numel() if divisor is None else divisor), 1.0, _lib.ptr(out),
              _lib.ptr(plan.workspace), _lib.stream_ptr())


def _ssim(lib, plan, hr, out, weight=LAM, divisor=None, accumulate=0, scratch=None):
    from m2trans_amd import _lib
    if scratch is None:
        scratch = _scratch(lib, hr.shape[0], 3, hr.shape[-2], hr.shape[-1])
    rc = lib.m2t_ssim_loss(plan.handle, _lib.ptr(hr), weight, float(_n_map(hr) if divisor is None else divisor), 1.0, _lib.ptr(out),
                           accumulate, _lib.ptr(scratch), _lib.ptr(plan.workspace), _lib.stream_ptr())
    torch.cuda.synchronize()             # (the scratch of this helper dies with the call)
    return rc


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("scale,shape", [(2, (2, 40, 56)), (3, (2, 40, 56)), (4, (2, 40, 56)), (4, (2, 64, 96))])
def test_plan_entry_adds_the_seed_against_fp64(dtype, scale, shape):
    """m2t_pixel_loss(weight 0) then m2t_ssim_loss: ws:gpre against the restatement on the read-back bits of ws:srpre; then with the L1
    weight 1 the sum of both references (the L1 seed being sign(d) * (float)(1 / N), include/m2t.h)."""
    _lib, lib = _lib_()
    B, H, W = shape
    model = _model(scale, dtype)
    x, hr = _images(B, H, W, scale)
    plan = model._plan_for(x)
    _forward(lib, model, plan, x)
    torch.cuda.synchronize()
    pre = _srpre(plan, B, scale).clone()
    _require_coverage(pre, hr, f"{dtype} x{scale} {shape}")
    Hs, Ws = hr.shape[-2:]
    assert tuple(pre.shape[-2:]) != (Hs, Ws) or shape != (2, 40, 56), "(2, 40, 56) is meant to be reflect-padded"
    pad = torch.ones(pre.shape, dtype=torch.bool)
    pad[..., :Hs, :Ws] = False
    clamped = ((pre < 0) | (pre > 1)).cpu()
    sc = LAM / _n_map(hr)
    want_loss, want = R.loss_and_seed(pre.cpu(), hr.cpu(), weight=LAM, divisor=_n_map(hr))
    l1, out = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)
    tag = f"{dtype} x{scale} {shape}"
    # the structural term alone
    gpre.fill_(float("nan"))
    assert _pixel(lib, plan, hr, l1, weight=0.0) == 0 and _ssim(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    assert bool(torch.isfinite(got).all()), tag
    assert int(torch.count_nonzero(got[pad])) == 0, f"{tag}: seed in the padding"
    assert int(torch.count_nonzero(got[clamped])) == 0, f"{tag}: seed where the clamp is active"
    assert int(torch.count_nonzero(want)) > 0.2 * hr.numel()
    nbad, worst = _gate(got, want, sc)
    print(f"{tag}: SSIM seed, largest excess over the gate {worst:.3e}; value {float(out):.9e} against {float(want_loss):.9e}")
    assert nbad == 0, f"{tag}: {nbad} seed elements beyond the gate, worst by {worst:.3e}"
    assert abs(float(out) - float(want_loss)) <= 1e-6 * abs(float(want_loss)), (tag, float(out), float(want_loss))
    # behind the L1 seed
    gpre.fill_(float("nan"))
    assert _pixel(lib, plan, hr, l1, weight=1.0) == 0 and _ssim(lib, plan, hr, out) == 0
    got = gpre.view(pre.shape).double().cpu()
    inner = pre[..., :Hs, :Ws].double().cpu()
    d = inner.clamp(0.0, 1.0) - hr.double().cpu()
    seed_l1 = torch.zeros_like(want)
    seed_l1[..., :Hs, :Ws] = RP.derivative("l1", d) * RP.clamp_mask(inner) * float(torch.tensor(1.0 / hr.numel(), dtype=torch.float32))
    nbad, worst = _gate(got, want, sc, prefill=seed_l1)
    assert nbad == 0, f"{tag}: {nbad} elements of L1 + SSIM beyond the gate, worst by {worst:.3e}"
    assert int(torch.count_nonzero(got[pad])) == 0 and int(torch.count_nonzero(got[clamped])) == 0, tag


def test_plan_entry_state_and_argument_errors():
    """State rules of m2t_add_output_grad.  An SR image below 11 x 11 cannot reach m2t_ssim_loss through a plan (m2t_plan_create pads
    the LR image to a multiple of 32 by reflection and so refuses anything below 17 x 17, i.e. 34 x 34 SR pixels at x2): the test
    requires that refusal, and M2T_ERR_ARG from the same routine through the plan-free entry."""
    _lib, lib = _lib_()
    model = _model(4, "fp32", 1)
    x, hr = _images(1, 32, 32, 4)
    plan = model._plan_for(x)
    out = torch.zeros(1, device="cuda")
    assert _ssim(lib, plan, hr, out) == STATE                        # before a forward
    _forward(lib, model, plan, x)
    assert _ssim(lib, plan, hr, out) == STATE                        # before any seed
    assert _pixel(lib, plan, hr, out, deferred=True) == 0
    assert _ssim(lib, plan, hr, out) == STATE                        # a deferred request leaves no materialised seed
    assert b"materialised" in lib.m2t_last_error_string()
    assert _pixel(lib, plan, hr, out) == 0
    assert _ssim(lib, plan, hr, out) == 0
    scratch = _scratch(lib, 1, 3, 128, 128)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    for bad in (dict(hr=None), dict(out=None), dict(scratch=None), dict(ws=None), dict(R=0.0), dict(div=0.0), dict(div=float("nan"))):
        a = dict(hr=_lib.ptr(hr), out=_lib.ptr(out), scratch=_lib.ptr(scratch), ws=ws, R=1.0, div=float(_n_map(hr)))
        a.update(bad)
        assert lib.m2t_ssim_loss(plan.handle, a["hr"], LAM, a["div"], a["R"], a["out"], 0, a["scratch"], a["ws"], st) == ARG, bad
    torch.cuda.synchronize()
    h = C.c_void_p()
    assert lib.m2t_plan_create(C.byref(h), 1, 5, 5, 2, 1, _lib.F32) == ARG        # 10 x 10 SR pixels: no such plan
    small = torch.zeros(1, 3, 10, 16, device="cuda")
    assert lib.m2t_ssim_loss_scratch_bytes(1, 3, 10, 16) == 0
    assert lib.m2t_ssim_loss_tensor(_lib.ptr(small), _lib.ptr(small), 1, 3, 10, 16, 3 * 160, 16, 1.0, 1, 1.0, None, _lib.ptr(out), 0,
                                    _lib.ptr(scratch), st) == ARG


# ------------------------------------------------------------------ 4. TrainStep against the sequence by hand and against autograd
def _by_hand(model, plan, x, hr, lam=LAM, pix_div=None, ssim_div=None):
    """(l1 [1], ssim [1], gradients): m2t_forward -> m2t_pixel_loss (l1) -> m2t_ssim_loss -> m2t_backward into fresh buffers."""
    _lib, lib = _lib_()
    l1, ss = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    grads = torch.full_like(model.flat_params, float("nan"))
    _forward(lib, model, plan, x)
    assert _pixel(lib, plan, hr, l1, divisor=pix_div) == 0
    assert _ssim(lib, plan, hr, ss, weight=lam, divisor=ssim_div) == 0
    _backward(lib, model, plan, x, grads)
    torch.cuda.synchronize()
    return l1, ss, grads


@pytest.mark.parametrize("dtype,scale,tol", [("bf16", 4, 1e-2), ("fp32", 2, 1e-5)])
def test_train_step_is_the_sequence_by_hand_and_matches_the_autograd_route(dtype, scale, tol):
    """Two steps with different batches: loss, gradients, parameters and moments bit-identical to m2t_forward -> m2t_pixel_loss ->
    m2t_ssim_loss -> m2t_backward -> m2t_adam_step on a twin.  The first step's gradients are also compared with the route a user had
    to take: sr = model(x), torch's L1 plus the fp32 torch form of the restatement, backward() -- rel-L2 1e-5 in fp32, 1e-2 in bf16,
    the figures test_train_step_matches_the_autograd_route_through_torchs_loss uses for the same dtypes."""
    from m2trans_amd.train_step import TrainStep
    _lib, lib = _lib_()
    B, H, W = 2, 40, 56
    m_a, m_b = _model(scale, dtype), _model(scale, dtype)
    ts = TrainStep(m_a, lr=1e-4, world_size=1, lambda_ssim=LAM)
    exp_avg, exp_avg_sq = torch.zeros_like(m_b.flat_params), torch.zeros_like(m_b.flat_params)
    first_grads = None
    for step in range(2):
        x, hr = _images(B, H, W, scale, step)
        loss = ts.step(x, hr)
        torch.cuda.synchronize()
        plan = m_b._plan_for(x)
        l1, ss, grads = _by_hand(m_b, plan, x, hr)
        if step == 0:
            _require_coverage(_srpre(plan, B, scale), hr, f"{dtype} x{scale}")
            first_grads = grads.clone()
        n = grads.numel()
        _lib.check(lib.m2t_adam_step(_lib.ptr(m_b.flat_params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), n, 1e-4, 0.9,
                                     0.999, 1e-8, step + 1, 1.0, _lib.stream_ptr()), "m2t_adam_step")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grads).all()) and float(ss) > 0 and float(l1) > 0
        assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.ssim_loss, ss) and torch.equal(loss, l1 + ss), (step, float(loss))
        assert ts.loss is loss
        assert_flat_equal(m_a, ts.grads, grads, f"gradients, step {step}")
        assert_flat_equal(m_a, m_a.flat_params.detach(), m_b.flat_params.detach(), f"parameters, step {step}")
        assert_flat_equal(m_a, ts.exp_avg, exp_avg, f"exp_avg, step {step}")
        assert_flat_equal(m_a, ts.exp_avg_sq, exp_avg_sq, f"exp_avg_sq, step {step}")
    # the autograd route, on the weights of step 0
    model = _model(scale, dtype)
    x, hr = _images(B, H, W, scale, 0)
    sr = model(x)
    want_loss = torch.nn.L1Loss()(sr, hr) + LAM * (1.0 - R.ssim_map(sr, hr)).mean()
    want_loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    got, want = [], []
    for nme, (o, k) in model.param_offsets().items():
        if named[nme].grad is None:
            continue
        want.append(named[nme].grad.reshape(-1).double().cpu())
        got.append(first_grads[o:o + k].double().cpu())
    got, want = torch.cat(got), torch.cat(want)
    assert float(want.norm()) > 0
    err = float((got - want).norm() / want.norm())
    print(f"{dtype} x{scale}: by-hand gradients against the autograd route, rel-L2 {err:.3e} (gate {tol:g})")
    assert err <= tol, (dtype, err)
    # the term is live: the L1 step alone gives other gradients
    ts0 = TrainStep(_model(scale, dtype), world_size=1)
    ts0.forward_backward(x, hr)
    torch.cuda.synchronize()
    assert not torch.equal(ts0.grads, first_grads)


# ------------------------------------------------------------------ 5. the default step is untouched
@pytest.mark.parametrize("dtype,scale", [("bf16", 4), ("fp32", 2)])
def test_lambda_ssim_zero_is_the_default_step_bit_for_bit(dtype, scale):
    from m2trans_amd.train_step import TrainStep
    B, H, W = 2, 40, 56
    res = []
    for kw in ({}, {"lambda_ssim": 0.0}):
        model = _model(scale, dtype)
        ts = TrainStep(model, lr=1e-4, world_size=1, **kw)
        assert ts.ssim_loss is None and ts._ssim_scratch == {}
        out = []
        for step in range(2):
            x, hr = _images(B, H, W, scale, step)
            loss = ts.step(x, hr)
            torch.cuda.synchronize()
            assert ts.ssim_loss is None and loss is ts.l1_loss
            out.append((loss.clone(), ts.grads.clone(), model.flat_params.detach().clone()))
        res.append((model, out))
    (model, a), (_, b) = res
    for step in range(2):
        assert torch.equal(a[step][0], b[step][0])
        assert_flat_equal(model, a[step][1], b[step][1], f"gradients, step {step}")
        assert_flat_equal(model, a[step][2], b[step][2], f"parameters, step {step}")


# ------------------------------------------------------------------ 6. accumulation
def test_accumulated_ssim_equals_the_micro_batch_gradients_summed_in_call_order():
    """accum_steps = 2 at micro-batch (1, 40, 56), bf16 x4: the accumulated buffer is the fp32 sum, in call order, of the two micro-batch
    gradients taken by hand with the cycle's divisors (the rule of tests/test_gpu_accum.py); ts.ssim_loss is the sum of the two values."""
    from m2trans_amd._lib import M2TError
    from m2trans_amd.train_step import TrainStep
    H, W = 40, 56
    x, hr = _images(2, H, W, 4)
    m_a, m_b = _model(4, "bf16"), _model(4, "bf16")
    ts = TrainStep(m_a, world_size=1, accum_steps=2, lambda_ssim=LAM)
    ts.forward_backward(x[0:1], hr[0:1])
    with pytest.raises(M2TError):
        ts.optimizer_step()                                          # in mid-cycle
    with pytest.raises(M2TError):
        ts.set_lambda_ssim(0.0)
    loss = ts.forward_backward(x[1:2], hr[1:2])
    torch.cuda.synchronize()
    parts = []
    for i in range(2):
        cx, chr_ = x[i:i + 1].contiguous(), hr[i:i + 1].contiguous()
        parts.append(_by_hand(m_b, m_b._plan_for(cx), cx, chr_, pix_div=hr.numel(), ssim_div=_n_map(hr)))
    assert float(parts[1][2].abs().max()) > 0 and float(parts[1][1]) > 0
    assert torch.equal(ts.ssim_loss, parts[0][1] + parts[1][1]), (float(ts.ssim_loss), float(parts[0][1] + parts[1][1]))
    assert torch.equal(ts.l1_loss, parts[0][0] + parts[1][0])
    assert torch.equal(loss, ts.l1_loss + ts.ssim_loss)
    assert_flat_equal(m_a, ts.grads, parts[0][2] + parts[1][2], "accumulated L1 + SSIM")
    ts.optimizer_step()
    assert ts.micro_count == 0


# ------------------------------------------------------------------ 7. with the differentiable SemanticLoss
def test_semantic_grad_route_adds_the_three_contributions():
    """TrainStep(lambda_ssim, differentiable SemanticLoss) against the sequence by hand (m2t_forward -> encoder value and gradient ->
    m2t_pixel_loss -> m2t_ssim_loss -> m2t_add_output_grad -> m2t_backward): bit-identical.  And the seed after the three contributions
    against the three taken alone: two fp32 adds, each within half an ulp of its partial sum -> 2e-7 (|a| + |b| + |c|) per element."""
    from m2trans_amd.losses import SemanticLoss
    from m2trans_amd.train_step import TrainStep
    from oracle import swin_oracle as S
    _lib, lib = _lib_()
    scale, nb, B, H, W = 4, 1, 2, 64, 64                         # (the shape of tests/test_gpu_semantic_grad.py's _model_and_inputs)
    x, hr = _images(B, H, W, scale)
    sl = SemanticLoss(criterion="l1", N_patches=3, device="cuda", compute_dtype="bf16", max_batch=4, differentiable=True)
    sl.load_image_encoder(S.closed_form_swin_params())
    g = torch.Generator().manual_seed(8)
    sl.set_text_features({"a": torch.randn(512, generator=g), "b": torch.randn(512, generator=g)})
    caps = ["a", "b"]
    m_a, m_b = _model(scale, "bf16", nb), _model(scale, "bf16", nb)
    ts = TrainStep(m_a, world_size=1, semantic_loss=sl, lambda_clip=0.01, lambda_ssim=LAM)
    torch.manual_seed(1)
    loss = ts.forward_backward(x, hr, caps)
    torch.cuda.synchronize()
    # by hand
    plan = m_b._plan_for(x)
    ws, st = _lib.ptr(plan.workspace), _lib.stream_ptr()
    sr = torch.empty_like(hr)
    l1, ss = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    g_b = torch.full_like(m_b.flat_params, float("nan"))
    torch.manual_seed(1)
    _lib.check(lib.m2t_forward(plan.handle, _lib.ptr(m_b.flat_params), _lib.ptr(x), _lib.ptr(sr), 1.0, 1, ws, st), "m2t_forward")
    _, gsem, origins = sl._value_and_grad(sr, hr, caps)
    gsem = gsem.contiguous()
    arr = None if origins is None else (C.c_int * (2 * len(origins)))(*[int(v) for o in origins for v in o])
    gpre = plan.ws_tensor("gpre", dtype=torch.float32)

    def seed(pixel_weight, with_ssim, with_sem):
        assert _pixel(lib, plan, hr, l1, weight=pixel_weight) == 0
        if with_ssim:
            assert _ssim(lib, plan, hr, ss) == 0
        if with_sem:
            _lib.check(lib.m2t_add_output_grad(plan.handle, _lib.ptr(gsem), gsem.shape[2], gsem.shape[3], arr, 0.01, 1.0, ws, st), "m2t_add_output_grad")
        torch.cuda.synchronize()
        return gpre.clone()

    a, b, c = seed(1.0, False, False), seed(0.0, True, False), seed(0.0, False, True)
    for t in (a, b, c):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    d = seed(1.0, True, True)
    a, b, c, d = (t.double().cpu() for t in (a, b, c, d))
    excess = (d - (a + b + c)).abs() - 2e-7 * (a.abs() + b.abs() + c.abs())
    assert float(excess.max()) <= 0.0, float(excess.max())
    _backward(lib, m_b, plan, x, g_b)
    torch.cuda.synchronize()
    assert torch.equal(ts.l1_loss, l1) and torch.equal(ts.ssim_loss, ss)
    assert torch.equal(loss, ts.l1_loss + ts.ssim_loss + ts.clip_loss)
    assert_flat_equal(m_a, ts.grads, g_b, "semantic-gradient route with the SSIM term")
